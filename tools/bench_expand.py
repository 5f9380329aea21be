#!/usr/bin/env python3
"""Corpus expansion on an NQ-shaped case: 334,314 x 768 rows of synth.make_corpus with clusters of 12; 190,727 of
them (about 57 % of every cluster) are the original corpus, the other 143,587 are permuted to the end and inserted — the shape of
the reference's NQ_ar2_334314_expand run (--docnum 190727).

Reports the centroid pass (ms, GB/s), the assignment (ms, TFLOP/s), the merge (us), the whole expansion (ms, host preparation and
read-back included), an online 64-doc GDRRetriever.add_documents (ms), and the reference's per-document loop restated in torch on
the CPU, timed on 1,000 rows and extrapolated.  Prints one JSON line last.

    python tools/bench_expand.py [--rows 334314] [--docnum 190727] [--reps 5]
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gdr_amd import codec, ops, synth                     # noqa: E402
from gdr_amd._ffi import check, lib, ptr, stream_ptr     # noqa: E402
from gdr_amd.modeling import GDRRetriever, expand_cluster_index   # noqa: E402


def timed(fn, reps):
    """median ms of fn() over reps runs (after one warm-up), device work included."""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def timed_dev(fn, reps):
    """median ms between device events around fn()."""
    fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=334314)
    ap.add_argument("--docnum", type=int, default=190727)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu_rows", type=int, default=1000)
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    N, d, csz = a.rows, a.d, 12
    rng = np.random.default_rng(0)
    full = synth.make_corpus(N, d, cluster_size=csz, seed=1)
    held = np.zeros(N, bool)
    held[rng.choice(N, N - a.docnum, replace=False)] = True
    order = np.concatenate([np.nonzero(~held)[0], rng.permutation(np.nonzero(held)[0])])   # originals first, in cluster order
    D = np.ascontiguousarray(full[order])
    del full
    n_cl = (N + csz - 1) // csz
    cl = order[:a.docnum] // csz                                                           # cluster of every original row
    offs = np.concatenate([[0], np.cumsum(np.bincount(cl, minlength=n_cl))]).astype(np.int32)
    mem = np.argsort(cl, kind="stable").astype(np.int32)
    names = ["-".join(str(x) for x in synth.cluster_digits(c, 4, 30)) for c in range(n_cl)]
    index = codec.ClusterIndex(names, offs, mem)
    Dd = torch.from_numpy(D).to(dev)
    n_new = N - a.docnum
    rows = index.unassigned(a.docnum, N)
    assert rows.size == n_new

    # centroid pass (the kernel alone: members sorted and uploaded beforehand)
    mem_s = torch.from_numpy(index.sorted_members()).to(dev)
    offs_d = torch.from_numpy(offs).to(dev)
    cent = torch.empty((n_cl, d), dtype=torch.float32, device=dev)
    cnt = torch.empty((n_cl,), dtype=torch.int32, device=dev)
    run_c = lambda: check(lib().gdr_cluster_centroids(ptr(Dd), N, d, ptr(offs_d), ptr(mem_s), int(mem.size), n_cl, ptr(cent),   # noqa: E731
                                                      ptr(cnt), stream_ptr()), "centroids")
    t_cent = timed_dev(run_c, a.reps)
    cent_bytes = (mem.size + n_cl) * d * 4
    fc = ops.FrozenCentroids.from_tensors(cent, cnt)
    n_live = fc.compact.shape[0]

    # skewed centroid pass: 2,000 clusters of 1-200 members and one of 8,300 over 20,000 rows (tests/test_gpu_expand.py's shape)
    sk_sizes = np.concatenate([rng.integers(1, 201, 2000), [8300]])
    sk_offs = torch.from_numpy(np.concatenate([[0], np.cumsum(sk_sizes)]).astype(np.int32)).to(dev)
    sk_mem = torch.from_numpy(np.concatenate([np.sort(rng.choice(20000, s_, replace=False)) for s_ in sk_sizes]).astype(np.int32)).to(dev)
    sk_cent = torch.empty((sk_sizes.size, d), dtype=torch.float32, device=dev)
    sk_cnt = torch.empty((sk_sizes.size,), dtype=torch.int32, device=dev)
    run_sk = lambda: check(lib().gdr_cluster_centroids(ptr(Dd), 20000, d, ptr(sk_offs), ptr(sk_mem), int(sk_mem.numel()),   # noqa: E731
                                                       int(sk_sizes.size), ptr(sk_cent), ptr(sk_cnt), stream_ptr()), "centroids")
    t_skew = timed_dev(run_sk, a.reps)

    # assignment
    X = Dd[a.docnum:]
    t_assign = timed_dev(lambda: fc.assign(X, compact=True), a.reps)
    flop = 2.0 * n_new * n_live * d
    tgt = fc.assign(X, compact=True)

    # merge
    ids = torch.from_numpy(rows).to(dev)
    mem_d = torch.from_numpy(mem).to(dev)
    t_merge = timed(lambda: ops.cluster_insert(offs_d, mem_d, ids, tgt, fc.cmap), a.reps)

    # whole expansion: host preparation, centroids, assignment, merge, one read-back of the CSR
    t_whole = timed(lambda: expand_cluster_index(Dd, index, rows), a.reps)

    # online: 64 documents into a live retriever (centroids already frozen)
    args = types.SimpleNamespace(kary=30, output_vocab_size=30, position=1)
    r = GDRRetriever(None, Dd[:a.docnum].clone(), index, args)
    r.add_documents(X[:64])
    ts, lo = [], 64
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r.add_documents(X[lo:lo + 64])
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
        lo += 64
    t_online = float(np.median(ts))

    # CPU baseline: the reference's per-document loop (main_models.py:283-293) in torch on the CPU, 1,000 rows, extrapolated
    cent_cpu = fc.compact.cpu()
    id_mapping = {names[c]: index[names[c]] for c in fc.cmap.cpu().tolist()}
    live_names = [names[c] for c in fc.cmap.cpu().tolist()]
    Xc = torch.from_numpy(D[a.docnum:a.docnum + a.cpu_rows])
    t0 = time.perf_counter()
    for i in range(Xc.shape[0]):
        sim = torch.mul(Xc[i], cent_cpu).sum(dim=-1)
        target = live_names[int(np.argmax(sim))]
        id_mapping[target].append(a.docnum + i)
        id_mapping[target] = list(set(id_mapping[target]))
    t_cpu_rows = (time.perf_counter() - t0) * 1e3
    t_cpu = t_cpu_rows * n_new / Xc.shape[0]

    print(f"corpus {N} x {d}, {n_cl} clusters of {csz} ({n_live} non-empty), {a.docnum} original rows, {n_new} inserted")
    print(f"centroid pass     {t_cent:9.3f} ms   {cent_bytes / t_cent / 1e6:8.1f} GB/s  ({cent_bytes / 1e6:.0f} MB)")
    print(f"  skewed          {t_skew:9.3f} ms   (2,000 clusters of 1-200 + one of 8,300 members)")
    n_chunks = -(-n_new // ops.ASSIGN_CHUNK)
    print(f"assignment        {t_assign:9.3f} ms   {flop / t_assign / 1e9:8.1f} TFLOP/s  ({flop / 1e12:.2f} TFLOP, {n_chunks} calls)")
    print(f"merge             {t_merge * 1e3:9.1f} us")
    print(f"whole expansion   {t_whole:9.3f} ms")
    print(f"online 64-doc add {t_online:9.3f} ms")
    print(f"CPU baseline      {t_cpu:9.0f} ms  (EXTRAPOLATED from {Xc.shape[0]} rows: {t_cpu_rows:.0f} ms; the reference's torch.cat "
          "build of the centroid matrix is not included)")
    print(json.dumps({"bench": "expand", "rows": N, "d": d, "clusters": n_cl, "live_clusters": n_live, "inserted": n_new,
                      "centroids_ms": round(t_cent, 4), "centroids_GBps": round(cent_bytes / t_cent / 1e6, 1),
                      "centroids_skewed_ms": round(t_skew, 4), "assign_calls": n_chunks,
                      "assign_ms": round(t_assign, 3), "assign_TFLOPs": round(flop / t_assign / 1e9, 2),
                      "merge_us": round(t_merge * 1e3, 1), "whole_ms": round(t_whole, 3), "online64_ms": round(t_online, 3),
                      "cpu_baseline_ms_extrapolated": round(t_cpu, 0), "cpu_rows_timed": int(Xc.shape[0]),
                      "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
