#!/usr/bin/env python3
"""Hierarchical k-means docid construction on an NQ-shaped case: 334,314 x 768 rows of synth.make_corpus,
k = c = 30 — the shape of the reference's `kmeans.py --k 30 --c 30` run behind the bert_k30_c30 ids.

Reports the three kernels of one root-level Lloyd round (assign / partition / centroids: ms between device events around many
rounds, against bytes / 5.5 TB/s), the same for the second level (k nodes), one k-means++ seeding step of the root, the whole build
for every --init in turn in one process (s, per-level rounds, the tree's inertia, and the seeding's share of the build from event
pairs around every seeding of a level) and, if sklearn is importable here, the reference's recipe (MiniBatchKMeans / KMeans,
n_init = 100) on a sub-sample, extrapolated and labelled so.  Prints one JSON line last.

    python tools/bench_kmeans.py [--rows 334314] [--n_init 4] [--init hash k-means++] [--reps 20] [--cpu_rows 20000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gdr_amd import kmeans, ops, synth                     # noqa: E402
from gdr_amd._ffi import lib                               # noqa: E402

HBM = 5.5e12     # B/s: gathered whole rows from HBM (the rate the byte floors are quoted against)


def timed_dev(fn, reps):
    """mean ms per call between one pair of device events around `reps` calls (after 3 warm-up calls)."""
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def round_kernels(D, rows, off, cent, k, reps):
    """ms of assign / partition / centroids for one Lloyd round of the level (rows, off) and their byte floors."""
    N, d = D.shape
    n, S = rows.numel(), off.numel() - 1
    ws = ops.Workspace(D.device)
    wa = ops.kmeans_worklist(off, lib().gdr_kmeans_assign_tile())
    wp = ops.kmeans_worklist(off, lib().gdr_kmeans_partition_tile())
    lab, _sc, _ch, _st = ops.kmeans_assign(D, rows, off, cent, k, work=wa, workspace=ws)
    crow, coff, _st = ops.kmeans_partition(rows, lab, off, k, work=wp, workspace=ws)
    t_a = timed_dev(lambda: ops.kmeans_assign(D, rows, off, cent, k, work=wa, prev_labels=lab, workspace=ws), reps)
    t_p = timed_dev(lambda: ops.kmeans_partition(rows, lab, off, k, work=wp, workspace=ws), reps)
    ws_c = ops.Workspace(D.device)
    t_c = timed_dev(lambda: ops.kmeans_centroids(D, coff, crow, workspace=ws_c), reps)
    t_seq = timed_dev(lambda: ops.cluster_centroids_csr(D, coff, crow, n), reps)
    row_bytes = n * d * 4
    sizes = (coff[1:] - coff[:-1])
    return {"nodes": S, "rows": n, "assign_ms": round(t_a, 4), "assign_floor_ms": round((row_bytes + n * 16) / HBM * 1e3, 4),
            "partition_ms": round(t_p, 4), "partition_floor_ms": round(n * 16 / HBM * 1e3, 5),
            "centroids_ms": round(t_c, 4), "centroids_floor_ms": round(row_bytes / HBM * 1e3, 4),
            "sequential_centroids_ms": round(t_seq, 4),
            "largest_child": int(sizes.max().item())}, (crow, coff)


def seed_step(D, rows, off, k, reps):
    """ms of one gdr_kmeans_seed_dist step over the level (T candidates per node) and its byte floor (the rows once)."""
    n, S, T = rows.numel(), off.numel() - 1, kmeans.n_trials(k)
    work = ops.kmeans_worklist(off, lib().gdr_kmeans_seed_tile())
    cand = rows[(off[:-1, None].long() + torch.arange(T, device=D.device)[None, :] % (off[1:] - off[:-1])[:, None].long())]
    d2 = torch.full((n,), float("inf"), device=D.device)
    e = torch.zeros((S,), dtype=torch.int32, device=D.device)
    t = timed_dev(lambda: ops.kmeans_seed_dist(D, rows, off, cand, d2, e, work=work), reps)
    return {"nodes": S, "rows": n, "trials": T, "seed_dist_ms": round(t, 4),
            "seed_dist_floor_ms": round((n * D.shape[1] * 4 + n * 4 * (1 + T)) / HBM * 1e3, 4)}


class SeedingClock:
    """Event pairs around every kmeans.seed_level call of a build: the device time the seeding of the levels takes."""

    def __enter__(self):
        self.pairs, self.orig = [], kmeans.seed_level

        def timed(*a, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = self.orig(*a, **kw)
            e1.record()
            self.pairs.append((e0, e1))
            return out
        kmeans.seed_level = timed
        return self

    def __exit__(self, *exc):
        kmeans.seed_level = self.orig

    def ms(self):
        torch.cuda.synchronize()
        return sum(a.elapsed_time(b) for a, b in self.pairs)


def cpu_reference(X, k, c, threads):
    """The reference's recipe through sklearn on X: seconds for the root split and for the whole recursion."""
    from sklearn.cluster import KMeans, MiniBatchKMeans
    try:
        from threadpoolctl import threadpool_limits
    except ImportError:
        threadpool_limits = None
    km = KMeans(n_clusters=k, max_iter=300, n_init=100, init="k-means++", random_state=7, tol=1e-7)
    mb = MiniBatchKMeans(n_clusters=k, max_iter=300, n_init=100, init="k-means++", random_state=3, batch_size=1000,
                         reassignment_ratio=0.01, max_no_improvement=20, tol=1e-7)

    def rec(pos, root):
        if not root and len(pos) <= c:
            return
        pred = (mb if len(pos) >= 1000 else km).fit_predict(X[pos])
        for j in range(k):
            child = pos[pred == j]
            if len(child) and len(child) < len(pos):
                rec(child, False)

    import contextlib
    t0 = time.perf_counter()
    with (threadpool_limits(limits=threads) if threadpool_limits else contextlib.nullcontext()):
        rec(np.arange(X.shape[0]), True)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=334314)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--k", type=int, default=30)
    ap.add_argument("--c", type=int, default=30)
    ap.add_argument("--n_init", type=int, default=kmeans.DEFAULT_N_INIT)
    ap.add_argument("--init", nargs="+", default=list(kmeans.INITS), choices=kmeans.INITS, help="the seedings to build with, in turn")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu_rows", type=int, default=20000, help="sub-sample for the sklearn line (0: skip)")
    ap.add_argument("--max_depth", type=int, default=12)
    ap.add_argument("--kernels_only", action="store_true", help="one pass over the kernels of a root round (for a profiler run)")
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    N, d, k = a.rows, a.d, a.k
    X = synth.make_corpus(N, d, seed=1)
    D = torch.from_numpy(X).to(dev)
    rows = torch.arange(N, dtype=torch.int32, device=dev)
    off = torch.tensor([0, N], dtype=torch.int32, device=dev)
    # a root state a few rounds into Lloyd (balanced children, as in the build), then the second level under it
    warm = kmeans.build_docids(D, k=k, c=N, seed=7, max_iter=5, n_init=1, max_depth=2)
    cent = torch.from_numpy(warm.root_centroids).to(dev)
    res = {"rows": N, "d": d, "k": k, "c": a.c}
    res["root_round"], (crow, coff) = round_kernels(D, rows, off, cent, k, 3 if a.kernels_only else a.reps)
    if a.kernels_only:
        print(json.dumps(res))
        return
    live = (coff[1:] - coff[:-1]) > 0
    off2 = torch.cat([coff[:1], coff[1:][live]]).contiguous()
    S2 = off2.numel() - 1
    cent2 = D[crow.long()[(off2[:-1, None].long() + torch.arange(k, device=dev)[None, :] % (off2[1:] - off2[:-1])[:, None].long()).reshape(-1)]]
    res["level1_round"], _ = round_kernels(D, crow, off2, cent2.contiguous(), k, a.reps)
    res["level1_round"]["nodes"] = S2
    res["root_seed_step"] = seed_step(D, rows, off, k, a.reps)
    res["level1_seed_step"] = seed_step(D, crow, off2, k, a.reps)
    for n_init in sorted({1, a.n_init}):
        for init in a.init:
            kmeans.build_docids(D[:20000].contiguous(), k=k, c=a.c, n_init=1, max_depth=a.max_depth, init=init)     # warm-up
            torch.cuda.synchronize()
            with SeedingClock() as clock:
                t0 = time.perf_counter()
                out = kmeans.build_docids(D, k=k, c=a.c, seed=7, n_init=n_init, max_depth=a.max_depth, init=init)
                torch.cuda.synchronize()
                sec = time.perf_counter() - t0
                seed_ms = clock.ms()
            key = f"build_n_init_{n_init}" + ("" if init == "hash" else "_kmeans_pp")
            res[key] = {"init": init, "seconds": round(sec, 3), "seeding_ms": round(seed_ms, 2), "seeding_share": round(seed_ms / 1e3 / sec, 4),
                        "clusters": len(out.cluster_index.names), "depth": int(out.lengths.max()), "inertia": out.inertia,
                        "levels": out.levels}
    if a.cpu_rows:
        try:
            import sklearn  # noqa: F401
        except ImportError:
            sklearn = None
        if sklearn is not None:
            n = min(a.cpu_rows, N)
            sub = np.ascontiguousarray(X[np.random.default_rng(0).choice(N, n, replace=False)]).astype(np.float64)
            sec = cpu_reference(sub, k, a.c, 16)
            res["cpu_sklearn"] = {"rows": n, "seconds": round(sec, 2), "threads": 16,
                                  "extrapolated_seconds_full": round(sec * N / n, 1),
                                  "note": "reference recipe (n_init=100) on a sub-sample; full-size time extrapolated linearly in N"}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
