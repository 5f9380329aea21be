#!/usr/bin/env python3
"""Generate tests/golden/g14_expand.npz by running the REFERENCE's corpus expansion (TreeBuilder, encode_single_newid,
tree_embedding_calculate, tree_embedding_insert — main_models.py:112-179, 268-320) on CPU through make_golden's import shims.

Build-container only, like make_golden.py: only the arrays written here (inputs + the reference's outputs) are committed.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_expand.py
"""
import contextlib
import io
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True

import make_golden   # noqa: E402
import expand_ref    # noqa: E402

V, D_MODEL, N_ORIG, N_INS, SEED = 30, 64, 280, 100, 14


def make_names(rng):
    """~40 names of 1-3 digits (V = 30) where no name's token body is a prefix of another's (the reference's tree keeps the
    documents of a cluster on the node of its last token and would not descend below it): the first digit decides the length."""
    names = set()
    while len(names) < 8:
        names.add(str(rng.integers(0, 10)))
    while len(names) < 24:
        names.add("%d-%d" % (rng.integers(10, 20), rng.integers(0, V)))
    while len(names) < 42:
        names.add("%d-%d-%d" % (rng.integers(20, 30), rng.integers(0, V), rng.integers(0, V)))
    return sorted(names, key=lambda s: rng.random())


def main():
    rng = np.random.default_rng(SEED)
    torch.manual_seed(SEED)
    _pkg, mm, _mu, _mm = make_golden.import_reference()
    args = types.SimpleNamespace(kary=V, position=1, output_vocab_size=V, docnum=N_ORIG)
    names = make_names(rng)
    live = names[:-2]                                    # the last two clusters stay empty (never a candidate)
    # sizes: one big cluster (48), several singletons, the rest random
    sizes = np.zeros(len(names), np.int64)
    sizes[0] = 48
    sizes[1:6] = 1
    rest = N_ORIG - sizes.sum()
    k = len(live) - 6
    cut = np.sort(rng.choice(np.arange(1, rest), k - 1, replace=False))
    sizes[6:len(live)] = np.diff(np.concatenate([[0], cut, [rest]]))
    assert sizes.sum() == N_ORIG and (sizes[:len(live)] >= 1).all()
    cluster_of = rng.permutation(np.repeat(np.arange(len(names)), sizes))       # doc id -> cluster (original rows)

    # full-mantissa embeddings: per-cluster direction + noise; the inserted rows sit near a random live cluster
    base = rng.standard_normal((len(names), D_MODEL)).astype(np.float32) * 2.0
    D = np.empty((N_ORIG + N_INS, D_MODEL), np.float32)
    D[:N_ORIG] = base[cluster_of] + rng.standard_normal((N_ORIG, D_MODEL)).astype(np.float32)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    members = np.concatenate([rng.permutation(np.nonzero(cluster_of == c)[0]) for c in range(len(names))]).astype(np.int32)
    cent_r, counts_r = expand_ref.centroids(D, offsets, members)
    want = rng.integers(0, len(live), N_INS)
    want[:3] = 0                                          # the big cluster receives some
    i = 0
    while i < N_INS:                                      # resample until no inserted row is a near-tie
        x = (base[want[i]] + 1.5 * rng.standard_normal(D_MODEL)).astype(np.float32)
        _c, gap, band = expand_ref.assign(x[None], cent_r, counts_r)
        if gap[0] > 1000 * band[0]:
            D[N_ORIG + i] = x
            i += 1

    # the reference: tree over the original rows in doc-id order, centroids, then insertion of every row >= docnum
    builder = mm.TreeBuilder()
    for doc in range(N_ORIG):
        builder.add(mm.encode_single_newid(args, names[cluster_of[doc]]), doc)
    root = builder.build()
    emb = [torch.from_numpy(D[r].copy()) for r in range(D.shape[0])]
    mm.tree_embedding_calculate(root, emb)
    tok = {n: mm.encode_single_newid(args, n)[:-1] for n in names}
    ref_cent = np.zeros((len(names), D_MODEL), np.float32)
    for c, n in enumerate(live):
        cur = root
        for t in tok[n]:
            cur = cur.children[t]
        ref_cent[c] = cur.embedding.numpy()
    cluster_set = {"-".join(map(str, tok[n])) for n in live}
    id_mapping = {n: [int(x) for x in members[offsets[c]:offsets[c + 1]]] for c, n in enumerate(live)}
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        out = mm.tree_embedding_insert(root, id_mapping, emb, cluster_set, args)
    exp_mem = [np.sort(np.asarray(out.get(n, []), np.int32)) for n in names]
    exp_off = np.concatenate([[0], np.cumsum([m.size for m in exp_mem])]).astype(np.int32)
    exp_mem = np.concatenate(exp_mem).astype(np.int32)

    # the rules hold on these data
    assert np.array_equal(ref_cent.view(np.uint32), cent_r.view(np.uint32)), "sequential restatement != reference centroids"
    pairwise_differs = any(
        not np.array_equal((expand_ref.pairwise_sum(D[np.sort(members[offsets[c]:offsets[c + 1]])]) / np.float32(sizes[c])).view(np.uint32),
                           cent_r[c].view(np.uint32)) for c in range(len(live)) if sizes[c] > 2)
    assert pairwise_differs, "a pairwise sum gives the same centroids everywhere"
    tgt, gap, band = expand_ref.assign(D[N_ORIG:], cent_r, counts_r)
    assert (gap > 1000 * band).all()
    mo, mm_ = expand_ref.merge(offsets, members, np.arange(N_ORIG, N_ORIG + N_INS), tgt)
    assert expand_ref.as_sets(mo, mm_) == expand_ref.as_sets(exp_off, exp_mem), "restated insertion != reference"
    recv = np.bincount(tgt, minlength=len(names))
    assert (recv[:len(live)] == 0).any() and recv[0] >= 3, "want a live cluster that receives nothing and the big one receiving"

    path = os.path.join(HERE, "g14_expand.npz")
    np.savez(path, D=D, docnum=np.int64(N_ORIG), names=np.array(names), offsets=offsets, members=members,
             ref_centroids=ref_cent, exp_offsets=exp_off, exp_members=exp_mem, gap=gap)
    print(path, os.path.getsize(path), "bytes;", len(names), "clusters,", N_INS, "inserted")


if __name__ == "__main__":
    main()
