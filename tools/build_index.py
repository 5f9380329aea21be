#!/usr/bin/env python3
"""Docids and the cluster index from corpus embeddings, on the GPU — the role of the reference's
Data_process/NQ_dataset/kmeans/kmeans.py (`--k 30 --c 30` for the bert_k30_c30 ids), the counterpart of tools/embed_corpus.py
(which writes the embeddings) and tools/convert_artifacts.py (which converts an index somebody else built).

Input: X.npy fp32[N, d] (the concatenated doc_embed shards).  Output: `clusters.npz` in the layout ClusterIndex.save_npz /
convert_artifacts.py write (cluster_names, cluster_offsets, cluster_members) — what `--cluster_index`, GDRRetriever and
add_documents read — and optionally the id mapping (the reference's IDMapping pickle content) as npz: digits int32[N, depth]
(-1 padded) and lengths int32[N].

    python tools/build_index.py --embeddings doc_embed.npy --k 30 --c 30 --max_output_length 10 --out clusters.npz [--init k-means++]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gdr_amd import kmeans                                  # noqa: E402


def parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--embeddings", required=True, help="fp32 [N, d] .npy")
    ap.add_argument("--k", type=int, default=30)
    ap.add_argument("--c", type=int, default=30)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--n_init", type=int, default=kmeans.DEFAULT_N_INIT)
    ap.add_argument("--init", default="hash", choices=kmeans.INITS, help="seeding of every split: hashed member rows, or greedy k-means++ on the GPU")
    ap.add_argument("--max_iter", type=int, default=300)
    ap.add_argument("--max_output_length", type=int, default=10,
                    help="the model's --max_output_length: ids may have at most max_output_length - 2 digits (START and EOS)")
    ap.add_argument("--kary", type=int, default=30, help="the id scheme the index is for (0: no check of the digit range)")
    ap.add_argument("--output_vocab_size", type=int, default=None)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", required=True, help="clusters.npz")
    ap.add_argument("--idmapping", default="", help="also write the id mapping (digits, lengths) to this .npz")
    return ap


def main(argv=None):
    a = parser().parse_args(argv)
    torch.set_grad_enabled(False)
    X = np.load(a.embeddings)
    D = torch.from_numpy(X).to(a.device)
    t0 = time.time()
    out = kmeans.build_docids(D, k=a.k, c=a.c, seed=a.seed, max_iter=a.max_iter, n_init=a.n_init,
                              max_depth=kmeans.max_depth_for(a.max_output_length), kary=a.kary or None,
                              output_vocab_size=a.output_vocab_size, init=a.init)
    torch.cuda.synchronize()
    out.cluster_index.save_npz(a.out)
    if a.idmapping:
        with open(a.idmapping, "wb") as f:
            np.savez(f, digits=out.digits, lengths=out.lengths)
    print(json.dumps({"docs": int(X.shape[0]), "clusters": len(out.cluster_index.names), "depth": int(out.lengths.max()),
                      "inertia": out.inertia, "seconds": round(time.time() - t0, 3), "levels": out.levels}))


if __name__ == "__main__":
    main()
