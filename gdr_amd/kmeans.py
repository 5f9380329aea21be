"""Hierarchical k-means docids from corpus embeddings, on the device — the role of the reference's
Data_process/NQ_dataset/kmeans/kmeans.py (recursive sklearn k-means, `--k 30 --c 30` for the bert_k30_c30 ids).

The tree is built level by level: every open node of a level runs Lloyd's algorithm in the same launches
(gdr_kmeans_assign -> gdr_kmeans_partition -> gdr_kmeans_centroids per round).  The level loop, the restarts and the seeding
live here in torch; there is no per-node Python loop.  tests/kmeans_ref.py restates the semantics in numpy.  A split is seeded
from hashed member rows (init="hash", the default) or by the greedy k-means++ rule (init="k-means++": one gdr_kmeans_seed_dist
launch per step for the whole level; tests/kmeans_pp_ref.py restates it bit for bit).
"""
import math

import numpy as np
import torch

from . import codec, ops
from ._ffi import GdrError, lib

DEFAULT_N_INIT = 4            # smallest of {1, 2, 4, 8, 16} whose inertia is within 5 % of the reference's recipe
_M64 = (1 << 64) - 1


def _s64(x):
    """A 64-bit pattern as the Python int torch.int64 takes."""
    x &= _M64
    return x - (1 << 64) if x >> 63 else x


def _splitmix64_int(z):
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def _lsr(z, s):
    return (z >> s) & ((1 << (64 - s)) - 1)      # torch's >> on int64 is arithmetic


def _splitmix64_t(z):
    """splitmix64 of an int64 tensor (bit patterns; int64 multiplication wraps)."""
    z = z + _s64(0x9E3779B97F4A7C15)
    z = (z ^ _lsr(z, 30)) * _s64(0xBF58476D1CE4E5B9)
    z = (z ^ _lsr(z, 27)) * _s64(0x94D049BB133111EB)
    return z ^ _lsr(z, 31)


def _prefix(seed, restart, level):
    """The part of a key that does not depend on the document (tests/kmeans_ref.mix_prefix), as an int64 bit pattern."""
    h = _splitmix64_int(int(seed) & _M64)
    h = _splitmix64_int(h ^ (int(restart) & _M64))
    return _s64(_splitmix64_int(h ^ (int(level) & _M64)))


def mix_keys(seed, restart, level, doc_ids):
    """63-bit keys (int64 >= 0) of doc_ids (int64 tensor): splitmix64(prefix(seed, restart, level) ^ doc_id) >> 1 — integer
    operations only (int64 multiplication wraps), so the device agrees with tests/kmeans_ref.mix bit for bit."""
    return _lsr(_splitmix64_t(doc_ids ^ _prefix(seed, restart, level)), 1)


class DocIds:
    """Result of build_docids: digits int32[N, depth] (-1 padded), lengths int32[N], cluster_index (codec.ClusterIndex of the
    leaves, depth-first order), levels (per-level stats), inertia (sum over the splits of the chosen restart's inertia),
    root_centroids fp32[k, d] (the root split's final centroids: a warm start for a rebuild)."""

    def __init__(self, digits, lengths, cluster_index, levels, inertia, root_centroids=None):
        self.digits, self.lengths, self.cluster_index, self.levels, self.inertia = digits, lengths, cluster_index, levels, inertia
        self.root_centroids = root_centroids

    def id_mapping(self):
        """old id -> digit list: the content of the reference's IDMapping pickle."""
        return {i: self.digits[i, :self.lengths[i]].tolist() for i in range(self.digits.shape[0])}

    def docid_strings(self):
        return ["-".join(str(x) for x in self.digits[i, :self.lengths[i]]) for i in range(self.digits.shape[0])]


def max_depth_for(max_output_length):
    """Digits a decoded id can carry: generate() emits START, the body, EOS within max_output_length tokens
    (codec.encode_single_newid appends the EOS; ClusterIndex.token_bodies is the body)."""
    return int(max_output_length) - 2


def _segment_sum(v, off):
    """Per-segment sums of v (float64) over the CSR off (int64[S+1]) from one cumsum: a fixed order."""
    cs = torch.cat([v.new_zeros(1), torch.cumsum(v, 0)])
    return cs[off[1:]] - cs[off[:-1]]


def _lloyd(D, rows, node_off, cent, k, max_iter, work_a, work_p, ws, ws_c):
    """Lloyd over every node of the level from `cent` -> labels, score, rounds (updates done), status word (device), centroids."""
    n = rows.numel()
    labels = torch.full((n,), -1, dtype=torch.int32, device=rows.device)
    status = torch.zeros((1,), dtype=torch.int32, device=rows.device)
    rounds, done, score = 0, False, None
    for t in range(max_iter):
        new_labels, score, changed, st = ops.kmeans_assign(D, rows, node_off, cent, k, work=work_a, prev_labels=labels, workspace=ws)
        status |= st
        if int(changed.sum().item()) == 0:           # the one read-back of a round; round 0 always counts every row
            done = True
            break
        labels = new_labels
        crow, coff, st = ops.kmeans_partition(rows, labels, node_off, k, work=work_p, workspace=ws)
        status |= st
        new_cent, counts = ops.kmeans_centroids(D, coff, crow, workspace=ws_c)
        cent = torch.where((counts > 0)[:, None], new_cent, cent)   # an emptied child keeps its centroid
        rounds += 1
    if not done:
        labels, score, _changed, st = ops.kmeans_assign(D, rows, node_off, cent, k, work=work_a, prev_labels=labels, workspace=ws)
        status |= st
    return labels, score, rounds, status, cent


INITS = ("hash", "k-means++")
_W_MAX = float((1 << 22) - 1)


def n_trials(k):
    """Candidates per greedy k-means++ step: sklearn's 2 + int(log(k)) (2 .. 6 for k = 2 .. 64)."""
    return 2 + int(math.floor(math.log(k)))


def _weights(d2, e, node_of):
    """floor(min(d2 * 2^(22 - e), 2^22 - 1)) as int64: the exact power of two is built from its float64 bit pattern."""
    scale = ((1045 - e.to(torch.int64)) << 52).view(torch.float64)
    return torch.floor(torch.clamp(d2.double() * scale[node_of], max=_W_MAX)).to(torch.int64)


def _seed_plusplus(D, rows, node_off, off64, sizes, node_of, hashed, k, seed, restart, level, work, status):
    """Greedy k-means++ seeds of every node of the level (tests/kmeans_pp_ref.seed_node) -> doc ids int64[S, k].
    hashed int64[S, k] are the hashed rule's ids: the first centre, every centre of a node of <= k members, and the centres a node
    of zero potential still lacks.  One gdr_kmeans_seed_dist launch per step for the whole level; the integer prefix sums, the
    draws and the argmin are torch; no read-back."""
    dev = D.device
    n, S, T = rows.numel(), sizes.numel(), n_trials(k)
    lo, hi = off64[:-1], off64[1:]
    a = _splitmix64_t(rows[lo].to(torch.int64) ^ _prefix(seed, restart, level))   # per node: its smallest doc id under the prefix
    tile_node = work[:, 0].to(torch.int64)
    tile_off = torch.cat([lo.new_zeros(1), torch.cumsum(torch.bincount(tile_node, minlength=S), 0)])
    trials = torch.arange(T, device=dev)
    # the draws depend on (seed, restart, level, node, step, trial) alone: all k - 1 steps at once, as float64 u * 2^-53 (exact)
    steps = torch.arange(1, k, device=dev)
    u = _lsr(_splitmix64_t(a[None, :, None] ^ ((steps << 8)[:, None, None] | trials[None, None, :])), 11).double() * 2.0 ** -53

    def node_max(v):                                                             # per-tile maxima -> per node (a max is order-free)
        return torch.zeros((S,), dtype=torch.float32, device=dev).scatter_reduce_(0, tile_node, v, "amax")

    picks, zero = [], []
    cand = torch.full((S, T), -1, dtype=torch.int32, device=dev)
    cand[:, 0] = hashed[:, 0].to(torch.int32)
    d2 = torch.full((n,), float("inf"), dtype=torch.float32, device=dev)
    e = torch.zeros((S,), dtype=torch.int32, device=dev)
    cd, _pot, mx, st = ops.kmeans_seed_dist(D, rows, node_off, cand, d2, e, work=work)
    status |= st
    d2, dmax = cd[:, 0].contiguous(), node_max(mx[:, 0])
    for step in range(1, k):
        e = torch.frexp(dmax).exponent.to(torch.int32)
        w = _weights(d2, e, node_of)
        cs = torch.cumsum(w, 0)                                                  # int64: exact in any order
        base = cs[lo] - w[lo]
        pot = cs[hi - 1] - base
        thr = torch.floor(u[step - 1] * pot.double()[:, None]).to(torch.int64)
        thr = torch.minimum(thr, pot[:, None] - 1).clamp_(min=0)
        pos = torch.searchsorted(cs, (base[:, None] + thr).reshape(-1), right=True).view(S, T)
        pos = torch.minimum(torch.maximum(pos, lo[:, None]), hi[:, None] - 1)    # a node of zero potential draws nothing
        cand = rows[pos]
        cd, tpot, mx, st = ops.kmeans_seed_dist(D, rows, node_off, cand, d2, e, work=work)
        status |= st
        cp = torch.cat([tpot.new_zeros((1, T)), torch.cumsum(tpot, 0)])
        pots = cp[tile_off[1:]] - cp[tile_off[:-1]]                              # [S, T], < 2^53
        best = (pots * 8 + trials[None, :]).min(1).values & 7                    # the smallest potential, ties to the lower trial
        picks.append(cand.gather(1, best[:, None])[:, 0])
        zero.append(pot == 0)
        d2 = cd.gather(1, best[node_of][:, None])[:, 0].contiguous()
        dmax = node_max(mx.gather(1, best[tile_node][:, None])[:, 0])
    greedy = torch.stack(picks, 1).to(torch.int64)
    keep = (sizes <= k)[:, None] | torch.stack(zero, 1)                          # a small node; a node whose potential was 0
    return torch.cat([hashed[:, :1], torch.where(keep, hashed[:, 1:], greedy)], 1)


def seed_level(D, rows, node_off, k, seed=7, restart=0, level=0, init="hash", work=None):
    """Doc ids int64[S, k] of the initial centres of every node of a level (rows int32[n], ascending inside a node; node_off
    int32[S+1]) and the kernels' status word int32[1].  "hash": the k smallest (key, doc id) of the node, a node of m < k members
    repeats them (centre j = member j mod m).  "k-means++": the greedy rule from there (_seed_plusplus); work is the level's work
    list over gdr_kmeans_seed_tile() rows (built here when absent)."""
    if init not in INITS:
        raise GdrError(f"seed_level: init={init!r} (one of {', '.join(INITS)})")
    dev = rows.device
    n, S = rows.numel(), node_off.numel() - 1
    off64 = node_off.to(torch.int64)
    sizes = off64[1:] - off64[:-1]
    node_of = torch.repeat_interleave(torch.arange(S, device=dev), sizes, output_size=n)
    rows64 = rows.to(torch.int64)
    # rows are ascending inside a node, so two stable sorts order them by (node, key, doc id)
    keys = mix_keys(seed, restart, level, rows64)
    o1 = torch.sort(keys, stable=True).indices
    o2 = torch.sort(node_of[o1], stable=True).indices
    order = o1[o2]                                                    # positions, grouped by node, by (key, id) inside it
    j = torch.arange(k, device=dev)[None, :] % sizes[:, None]
    ids = rows64[order[off64[:-1, None] + j]]
    status = torch.zeros((1,), dtype=torch.int32, device=dev)
    if init == "k-means++":
        if work is None:
            work = ops.kmeans_worklist(node_off, lib().gdr_kmeans_seed_tile())
        ids = _seed_plusplus(D, rows, node_off, off64, sizes, node_of, ids, k, seed, restart, level, work, status)
    return ids, status


def build_docids(D, k=30, c=30, seed=7, max_iter=300, n_init=DEFAULT_N_INIT, max_depth=8, init_centroids=None, kary=None,
                 output_vocab_size=None, init="hash"):
    """Hierarchical k-means ids of the corpus D fp32[N, d] (device) -> DocIds.  k children per split (2..64), leaves of <= c
    docs, n_init restarts per split (the smaller inertia wins), ids of at most max_depth digits (GdrError beyond).
    init_centroids fp32[k, d] replaces the seeding of the root (one restart there).  With kary the ids must be printable in
    that scheme: max(k, c) <= output_vocab_size.  init: "hash" seeds a split from its k members with the smallest hashed keys;
    "k-means++" runs the greedy k-means++ rule on the device — Lloyd, the restarts and the id rules are the same."""
    if init not in INITS:
        raise GdrError(f"build_docids: init={init!r} (one of {', '.join(INITS)})")
    if not isinstance(D, torch.Tensor) or not D.is_cuda:
        raise GdrError("build_docids: D must be a CUDA (ROCm) tensor; there is no CPU path")
    if D.dtype != torch.float32:
        raise GdrError(f"build_docids: the corpus must be float32, got {D.dtype} (a bf16 corpus is not supported)")
    if D.dim() != 2 or D.shape[1] % 4 or not 4 <= D.shape[1] <= ops.KMEANS_MAX_D:
        raise GdrError(f"build_docids: d={D.shape[-1]} (needs d % 4 == 0, 4 <= d <= {ops.KMEANS_MAX_D})")
    N, d = D.shape
    if N >= 1 << 31:
        raise GdrError(f"build_docids: N={N} does not fit int32 doc ids")
    if N < 1:
        raise GdrError("build_docids: empty corpus")
    if not 2 <= int(k) <= ops.KMEANS_MAX_K:
        raise GdrError(f"build_docids: k={k} (needs 2 <= k <= {ops.KMEANS_MAX_K})")
    if c < 1 or n_init < 1 or max_iter < 1 or max_depth < 1:
        raise GdrError(f"build_docids: c={c}, n_init={n_init}, max_iter={max_iter}, max_depth={max_depth} must all be >= 1")
    if kary:
        V = int(output_vocab_size if output_vocab_size is not None else kary)
        if max(k, c) > V:
            raise GdrError(f"build_docids: max(k, c) = {max(k, c)} digits do not fit output_vocab_size={V} (kary={kary})")
    if init_centroids is not None:
        if not init_centroids.is_cuda or init_centroids.dtype != torch.float32 or tuple(init_centroids.shape) != (k, d):
            raise GdrError(f"build_docids: init_centroids must be a CUDA float32 tensor of shape {(k, d)}")
    D = D.contiguous()
    dev = D.device
    ws, ws_c = ops.Workspace(dev), ops.Workspace(dev)
    ta, tp = lib().gdr_kmeans_assign_tile(), lib().gdr_kmeans_partition_tile()
    ts = lib().gdr_kmeans_seed_tile()
    xn2 = torch.empty((N,), dtype=torch.float64, device=dev)
    for lo in range(0, N, 1 << 16):
        x = D[lo:lo + (1 << 16)].double()
        xn2[lo:lo + (1 << 16)] = (x * x).sum(1)

    digits = torch.full((N, max_depth), -1, dtype=torch.int32, device=dev)
    path_len = torch.zeros((N,), dtype=torch.int32, device=dev)       # digits of a doc's leaf path (its id without the rank digit)
    rows = torch.arange(N, dtype=torch.int32, device=dev)
    node_off = torch.tensor([0, N], dtype=torch.int32, device=dev)
    levels, total_inertia, level = [], 0.0, 0
    while rows.numel():
        n, S = rows.numel(), node_off.numel() - 1
        if level >= max_depth:
            big = int((node_off[1:] - node_off[:-1]).max().item())
            raise GdrError(f"build_docids: a node of {big} docs at depth {level} needs ids longer than max_depth={max_depth}")
        off64 = node_off.to(torch.int64)
        sizes = off64[1:] - off64[:-1]
        node_of = torch.repeat_interleave(torch.arange(S, device=dev), sizes, output_size=n)
        work_a, work_p = ops.kmeans_worklist(node_off, ta), ops.kmeans_worklist(node_off, tp)
        work_s = work_a if ts == ta else ops.kmeans_worklist(node_off, ts)
        rows64 = rows.to(torch.int64)
        xn2_rows = xn2[rows64]
        best_labels = best_inertia = None
        rounds_max = 0
        status = torch.zeros((1,), dtype=torch.int32, device=dev)
        restarts = 1 if (level == 0 and init_centroids is not None) else n_init
        for r in range(restarts):
            if level == 0 and init_centroids is not None:
                cent = init_centroids.contiguous().clone()
            else:
                ids, st = seed_level(D, rows, node_off, k, seed, r, level, init, work_s)
                status |= st
                cent = D[ids.reshape(-1)].contiguous()
            labels, score, rounds, st, cent = _lloyd(D, rows, node_off, cent, k, max_iter, work_a, work_p, ws, ws_c)
            status |= st
            rounds_max = max(rounds_max, rounds)
            inertia = _segment_sum(xn2_rows - 2.0 * score.double(), off64)       # |x - c|^2 = |x|^2 - 2 (x.c - |c|^2/2)
            if best_labels is None:
                best_labels, best_inertia = labels, inertia
                if level == 0:
                    root_centroids = cent
            else:
                if level == 0 and bool((inertia < best_inertia)[0].item()):
                    root_centroids = cent
                better = inertia < best_inertia                                   # ties keep the lower restart
                best_labels = torch.where(better[node_of], labels, best_labels)
                best_inertia = torch.where(better, inertia, best_inertia)
        labels = best_labels
        # rule 6: a split that leaves every row of a node in one child gives row i of the node child i % k
        first = labels[off64[:-1]]
        same = _segment_sum((labels == first[node_of]).double(), off64) == sizes.double()
        degenerate = same & (sizes > 1)
        rank = torch.arange(n, device=dev) - off64[:-1][node_of]
        labels = torch.where(degenerate[node_of], (rank % k).to(torch.int32), labels)

        crow, coff, st = ops.kmeans_partition(rows, labels, node_off, k, work=work_p, workspace=ws)
        status |= st
        if int(status.item()):
            raise GdrError(f"build_docids: level {level}: the kernels reported status {int(status.item())} (malformed level state)")
        coff64 = coff.to(torch.int64)
        csize = coff64[1:] - coff64[:-1]                                          # [S*k]
        child_of = torch.repeat_interleave(torch.arange(S * k, device=dev), csize, output_size=n)
        crow64 = crow.to(torch.int64)
        digits[crow64, level] = (child_of % k).to(torch.int32)
        leaf = csize <= c
        pos_leaf = leaf[child_of]
        path_len[crow64[pos_leaf]] = level + 1
        ranked = pos_leaf & (csize[child_of] > 1)
        if bool(ranked.any().item()):
            if level + 1 >= max_depth:
                big = int(csize[leaf].max().item())
                raise GdrError(f"build_docids: a leaf of {big} docs at depth {level + 1} needs ids longer than max_depth={max_depth}")
            rk = (torch.arange(n, device=dev) - coff64[:-1][child_of]).to(torch.int32)
            digits[crow64[ranked], level + 1] = rk[ranked]
        level_inertia = float(best_inertia.sum().item())
        total_inertia += level_inertia
        open_child = ~leaf
        levels.append({"level": level, "nodes": S, "rows": n, "restarts": restarts, "rounds": rounds_max, "init": init,
                       "inertia": level_inertia, "leaves": int((leaf & (csize > 0)).sum().item())})
        rows = crow[~pos_leaf].contiguous()
        osz = csize[open_child]
        node_off = torch.cat([osz.new_zeros(1), torch.cumsum(osz, 0)]).to(torch.int32)
        level += 1

    dg = digits.cpu().numpy()
    lengths = (dg >= 0).sum(1).astype(np.int32)
    depth = int(lengths.max())
    dg = np.ascontiguousarray(dg[:, :depth])
    return DocIds(dg, lengths, _cluster_index(dg, path_len.cpu().numpy()), levels, total_inertia, root_centroids.cpu().numpy())


def _cluster_index(dg, path_len):
    """codec.ClusterIndex of the leaves, depth-first (lexicographic) order: a doc's cluster is the first path_len digits of its
    id (the id without the rank digit), its name those digits joined with '-'; members ascending."""
    path = np.where(np.arange(dg.shape[1])[None, :] < path_len[:, None], dg, -1)
    u, inv = np.unique(path, axis=0, return_inverse=True)     # rows sort lexicographically; the pad -1 sorts before any digit
    inv = inv.reshape(-1)
    members = np.argsort(inv, kind="stable").astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum(np.bincount(inv, minlength=len(u)))]).astype(np.int32)
    names = ["-".join(str(x) for x in row[row >= 0]) for row in u]
    return codec.ClusterIndex(names, offsets, members)
