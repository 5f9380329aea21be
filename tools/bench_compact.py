"""What compacting a live corpus costs and buys: at N = 320 000, d = 768 fp32 with 10 %, 50 % and 90 % of the rows
dead at random and with one contiguous dead block,

    compact_ms       ops.compact_plan (plan + its one read-back) + RowCompaction.rows in place (gdr_rows_compact, default chunk)
    baseline_ms      the only compaction expressible without it: D[live_bool].contiguous() plus a host remap of the member CSR —
                     its peak extra memory is a second corpus (n_live rows), ours is the bounce buffer
    search_*         GDRRetriever.search at 512 and 32 queries BEFORE the compaction (masked, over N rows) and AFTER it (over n_new rows)

and a sweep of the bounce buffer's size (chunk_rows) at 50 % dead, from which the library default was chosen.  The variants
ALTERNATE in one process, each timed with a host clock around work that ends in a device synchronise (the corpus is restored
outside the timed window), medians and spread (min, max) after warm-up.  Prints one JSON line per case and, with --out, writes them.

    python tools/bench_compact.py --out profiles/compact.jsonl"""
import argparse
import json
import os
import statistics
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gdr_amd import _ffi, codec, ops, synth  # noqa: E402
from gdr_amd.modeling import GDRRetriever  # noqa: E402

SWEEP_MIB = (1, 2, 4, 8, 16, 32, 64, 128, 256)


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _stats(ts):
    return {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}


def _alternate(variants, prepare, iters, warmup):
    """variants: name -> callable; prepare() runs untimed before each call.  Returns name -> list of ms."""
    times = {n: [] for n in variants}
    for it in range(warmup + iters):
        for n, fn in variants.items():
            prepare()
            ms = _timed(fn)
            if it >= warmup:
                times[n].append(ms)
    return times


def _masks(N, rng):
    m = {f"random_{p}": rng.random(N) >= p / 100 for p in (10, 50, 90)}
    block = np.ones(N, bool)
    block[N // 4:N // 4 + N // 2] = False
    m["block_50"] = block
    return m


def _args(V):
    return types.SimpleNamespace(num_return_sequences=4, output_vocab_size=V, max_output_length=4, length_penalty=0.8, kary=V, position=1,
                                 score_rate=[0, 1.0], loss_func="tanh")


def _retriever(D, live, V, dev):
    """A retriever over D whose index holds the live rows only: V * V clusters of consecutive rows."""
    N = D.shape[0]
    names = ["-".join(str(x) for x in synth.cluster_digits(c, 2, V)) for c in range(V * V)]
    bounds = np.linspace(0, N, V * V + 1).astype(np.int64)
    mem = np.nonzero(live)[0].astype(np.int32)
    offs = np.searchsorted(mem, bounds).astype(np.int32)
    return GDRRetriever(None, D, codec.ClusterIndex(names, offs, mem), _args(V)), offs, mem


def _case(name, D0, live, k, iters, warmup, dev):
    N, d = D0.shape
    row_bytes = d * 4
    n_live = int(live.sum())
    live_d = torch.from_numpy(live).to(dev)
    L = ops.LiveRows.from_bool(live_d)
    D = D0.clone()
    old = np.nonzero(live)[0]
    moved = int((old != np.arange(n_live)).sum())
    r_before, offs, mem = _retriever(D0, live, 32, dev)
    keep = {}

    def ours():
        plan = ops.compact_plan(L)
        keep["out"] = plan.rows(D)
        keep["plan"] = plan

    def baseline():
        keep["base"] = D[live_d].contiguous()
        new_id = np.cumsum(live, dtype=np.int64) - 1                           # the host remap of the CSR
        keep["mem"] = new_id[mem].astype(np.int32)

    times = _alternate({"compact": ours, "baseline": baseline}, lambda: D.copy_(D0), iters, warmup)
    D.copy_(D0)
    ours()
    assert torch.equal(keep["out"], keep["base"]), "the in-place compaction is not D[live]"
    assert np.array_equal(keep["plan"].ids(torch.from_numpy(mem).to(dev)).cpu().numpy(), keep["mem"])
    # the search before (masked over N rows) and after (n_new rows), alternating
    r_after, _o, _m = _retriever(D0.clone(), live, 32, dev)
    r_after.compact_documents()
    assert r_after.doc_embed.shape[0] == n_live
    out = {"case": name, "N": N, "d": d, "n_live": n_live, "rows_moved": moved, "iters": iters,
           "compact_ms": _stats(times["compact"]), "baseline_ms": _stats(times["baseline"]),
           "payload_GBps": round(moved * row_bytes / statistics.median(times["compact"]) / 1e6, 1),
           "traffic_GBps": round(4 * moved * row_bytes / statistics.median(times["compact"]) / 1e6, 1),   # src -> bounce -> dst: two reads, two writes
           "extra_bytes_compact": int(_ffi.lib().gdr_rows_compact_workspace_bytes(row_bytes, 0)), "extra_bytes_baseline": n_live * row_bytes}
    for B in (512, 32):
        Q = torch.from_numpy(synth.make_queries(D0[:4096].cpu().numpy(), B, seed=2)[0]).to(dev)
        st = _alternate({"before": lambda: r_before.search(Q, k), "after": lambda: r_after.search(Q, k)}, lambda: None, iters, warmup)
        out[f"search_B{B}_before_ms"], out[f"search_B{B}_after_ms"] = _stats(st["before"]), _stats(st["after"])
    out["device"] = torch.cuda.get_device_name(0)
    return out


def _sweep(D0, live, iters, warmup, dev):
    """The in-place move alone (the plan is made once) for bounce buffers of SWEEP_MIB."""
    N, d = D0.shape
    row_bytes = d * 4
    plan = ops.compact_plan(ops.LiveRows.from_bool(torch.from_numpy(live).to(dev)))
    D = D0.clone()
    variants = {mib: (lambda c=max((mib << 20) // row_bytes, 1): plan.rows(D, chunk_rows=c)) for mib in SWEEP_MIB}
    times = _alternate(variants, lambda: D.copy_(D0), iters, warmup)
    return {"case": "chunk_sweep_random_50", "N": N, "d": d, "n_live": plan.n_new, "iters": iters,
            "move_ms_by_bounce_MiB": {str(mib): _stats(t) for mib, t in times.items()}, "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rows", type=int, default=320_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    D0 = torch.from_numpy(synth.make_corpus(a.rows, 768, seed=1)).to(dev)
    masks = _masks(a.rows, np.random.default_rng(3))
    lines = []
    jobs = [lambda: _sweep(D0, masks["random_50"], a.iters, a.warmup, dev)] + [lambda n=n, m=m: _case(n, D0, m, 100, a.iters, a.warmup, dev)
                                                                                for n, m in masks.items()]
    for job in jobs:
        lines.append(json.dumps(job()))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
