"""Numpy restatement (float64) of the hierarchical k-means docid construction of gdr_amd/kmeans.py — the
semantics the device build is tested against, and of the id rules of the reference's
Data_process/NQ_dataset/kmeans/kmeans.py:41-90.  No sklearn, no torch.

A node is an ascending array of doc ids.  The root is always split; below it a node with <= c docs is a leaf.  A split is Lloyd's
algorithm from k member rows chosen by an integer hash, the best of n_init restarts by inertia.
"""
import numpy as np

M64 = (1 << 64) - 1


def splitmix64(z):
    """The splitmix64 finaliser on Python ints or uint64 arrays (wrapping arithmetic)."""
    if isinstance(z, np.ndarray):
        with np.errstate(over="ignore"):
            z = z.astype(np.uint64) + np.uint64(0x9E3779B97F4A7C15)
            z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            return z ^ (z >> np.uint64(31))
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def mix_prefix(seed, restart, level):
    """The part of mix() that does not depend on the document (a Python int < 2^64)."""
    h = splitmix64(int(seed) & M64)
    h = splitmix64(h ^ (int(restart) & M64))
    return splitmix64(h ^ (int(level) & M64))


def mix(seed, restart, level, doc_ids):
    """63-bit keys (int64 >= 0) of the documents: splitmix64(prefix ^ doc_id) >> 1.  Integer operations only."""
    z = np.asarray(doc_ids).astype(np.uint64) ^ np.uint64(mix_prefix(seed, restart, level))
    return (splitmix64(z) >> np.uint64(1)).astype(np.int64)


def init_rows(ids, k, seed, restart, level):
    """Doc ids of the k initial centroids of a node: its members with the k smallest keys, in (key, doc id) order; a node with
    m < k members repeats them (centroid j = member j mod m)."""
    keys = mix(seed, restart, level, ids)
    order = np.lexsort((ids, keys))
    return ids[order[np.arange(k) % len(ids)]]


def assign(X, C):
    """labels (ties to the lower j), best score x.c - |c|^2/2, and the gap to the second-best score, all float64."""
    s = X @ C.T - 0.5 * (C * C).sum(1)[None, :]
    lab = s.argmax(1)
    srt = np.sort(s, axis=1)
    return lab, srt[:, -1], srt[:, -1] - srt[:, -2]


def update(X, lab, C):
    """Member means; a centroid that received no row keeps its value (sklearn would relocate it: a deliberate deviation)."""
    C = C.copy()
    for j in range(C.shape[0]):
        m = lab == j
        if m.any():
            C[j] = X[m].sum(0) / m.sum()
    return C


def lloyd(X, C0, max_iter=300, on_round=None):
    """Lloyd from C0: assign / update until no label changes or max_iter updates are done, then a final assign — what
    sklearn's KMeans(init=C0, n_init=1, algorithm='lloyd', tol=0, max_iter=T) returns while no cluster empties.
    -> labels, centres, inertia, rounds (= updates).  on_round(t, gap, labels) sees every assign pass."""
    X = np.asarray(X, np.float64)
    C = np.asarray(C0, np.float64).copy()
    prev, rounds, done = None, 0, False
    for t in range(max_iter):
        lab, _best, gap = assign(X, C)
        if on_round:
            on_round(t, gap, lab)
        if prev is not None and np.array_equal(lab, prev):
            done = True
            break
        C = update(X, lab, C)
        prev, rounds = lab, rounds + 1
    if not done:
        lab, _best, gap = assign(X, C)
        if on_round:
            on_round(max_iter, gap, lab)
    inertia = float(((X - C[lab]) ** 2).sum())
    return lab, C, inertia, rounds


def split_node(X, ids, k, seed, level, max_iter, n_init, init_centroids=None, on_round=None, on_restart=None):
    """Labels of one node: the restart with the smallest inertia (ties to the lower restart), then rule 6 (a split that leaves
    every row in one child gives row i of the node child i % k).  -> labels, inertia."""
    Xn = np.asarray(X[ids], np.float64)
    best = None
    for r in range(1 if init_centroids is not None else n_init):
        C0 = init_centroids if init_centroids is not None else np.asarray(X[init_rows(ids, k, seed, r, level)], np.float64)
        lab, _C, inertia, _rounds = lloyd(Xn, C0, max_iter, (lambda t, g, l, r=r: on_round(r, t, g, l)) if on_round else None)
        if on_restart:
            on_restart(r, inertia)
        if best is None or inertia < best[1]:
            best = (lab, inertia)
    lab, inertia = best
    if len(ids) > 1 and (lab == lab[0]).all():
        lab = np.arange(len(ids)) % k
    return lab, inertia


def assemble_ids(n_docs, k, c, split_labels, max_depth=None):
    """The id rules (kmeans.py:41-90) over a label source: split_labels(ids, level, path) -> the node's labels.  A doc's id is
    the child digits on its path plus, in a leaf of 2..c docs, its rank in the leaf; a leaf of one doc gets no rank digit; a
    child that received no doc does not exist.  -> (ids: list of digit lists, leaves: [(path tuple, ascending doc ids)] in
    depth-first (lexicographic) order)."""
    digits = [[] for _ in range(n_docs)]
    leaves = []

    def put(doc, x, size, depth):
        if max_depth is not None and len(digits[doc]) >= max_depth:
            raise ValueError(f"a node of {size} docs at depth {depth} needs ids longer than max_depth={max_depth}")
        digits[doc].append(int(x))

    def visit(ids, level, path, force):
        if not force and len(ids) <= c:
            if len(ids) > 1:
                for rank, doc in enumerate(ids):
                    put(doc, rank, len(ids), level)
            leaves.append((path, ids))
            return
        lab = np.asarray(split_labels(ids, level, path))
        for j in range(k):
            child = ids[lab == j]
            if len(child) == 0:
                continue
            for doc in child:
                put(doc, j, len(ids), level)
            visit(child, level + 1, path + (j,), False)

    visit(np.arange(n_docs, dtype=np.int64), 0, (), True)
    return digits, leaves


def build(X, k, c, seed=7, max_iter=300, n_init=1, max_depth=None, init_centroids=None, on_round=None, on_restart=None,
          stats=None):
    """The whole tree.  on_round(path, restart, t, gap, labels) / on_restart(path, restart, inertia) observe every pass (the
    golden recipe checks its margins there); stats (a dict) receives the summed inertia of the chosen splits."""
    X = np.asarray(X)
    total = [0.0]

    def split_labels(ids, level, path):
        lab, inertia = split_node(
            X, ids, k, seed, level, max_iter, n_init, init_centroids if level == 0 else None,
            (lambda r, t, g, l: on_round(path, r, t, g, l)) if on_round else None,
            (lambda r, i: on_restart(path, r, i)) if on_restart else None)
        total[0] += inertia
        return lab

    out = assemble_ids(X.shape[0], k, c, split_labels, max_depth)
    if stats is not None:
        stats["inertia"] = total[0]
    return out


def cluster_csr(leaves):
    """names ('-'-joined path digits), offsets, members of the leaves, in their order."""
    names = ["-".join(str(x) for x in p) for p, _ in leaves]
    offsets = np.concatenate([[0], np.cumsum([len(m) for _, m in leaves])]).astype(np.int32)
    members = np.concatenate([m for _, m in leaves]).astype(np.int32)
    return names, offsets, members


def pad_digits(digits):
    """digits int32[N, depth] (-1 padded) and lengths int32[N] of a list of digit lists."""
    lens = np.array([len(x) for x in digits], np.int32)
    out = np.full((len(digits), int(lens.max()) if len(digits) else 0), -1, np.int32)
    for i, x in enumerate(digits):
        out[i, :len(x)] = x
    return out, lens


def two_stage_mean(D, members, chunk=256):
    """fp32 mean of D[members] as gdr_kmeans_centroids forms it: chunks of `chunk` members from the start of the list, each summed
    member after member in fp32 from 0, the chunk sums added in chunk order (a single chunk: its sum as is), one fp32 division."""
    D = np.asarray(D, np.float32)
    sums = []
    for lo in range(0, len(members), chunk):
        acc = np.zeros(D.shape[1], np.float32)
        for m in members[lo:lo + chunk]:
            acc = acc + D[m]
        sums.append(acc)
    if len(sums) == 1:
        total = sums[0]
    else:
        total = np.zeros(D.shape[1], np.float32)
        for v in sums:
            total = total + v
    return total / np.float32(len(members))
