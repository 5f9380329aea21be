"""What the live-row mask of the corpus search costs: gdr_sim_topk / gdr_sim_topk_bf16 with and without
GDR_SIM_LIVE_MASK at config C2's shape (N = 320 000, d = 768, k = 100, 1 000 random dead rows), the two calls ALTERNATING in
one process, each between device events, medians after warm-up.  The flagged time includes the copy of the bitmap into the
workspace, as ops.sim_topk issues it.  Prints one JSON line per case and, with --out, writes them to a file.

    python tools/bench_live_search.py --out profiles/live_search.jsonl"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gdr_amd import _ffi, ops, synth  # noqa: E402


def _case(name, B, D32, k, dead, bf16, iters, warmup, dev):
    N, d = D32.shape
    Q = torch.from_numpy(synth.make_queries(D32[:4096].cpu().numpy(), B, seed=2)[0]).to(dev)
    D = D32
    if bf16:
        D, Q = ops.to_bf16(D32), ops.to_bf16(Q)
    live = np.ones(N, bool)
    live[np.random.default_rng(3).choice(N, dead, replace=False)] = False
    L = ops.LiveRows.from_bool(torch.from_numpy(live).to(dev))
    ws = ops.Workspace(dev)
    calls = {"plain": lambda: ops.sim_topk(Q, D, k, workspace=ws, exact_on_overflow=False, return_status=True),
             "masked": lambda: ops.sim_topk(Q, D, k, workspace=ws, exact_on_overflow=False, return_status=True, live=L)}
    times = {n: [] for n in calls}
    launches = {}
    for n, call in calls.items():
        c0 = _ffi.lib().gdr_launch_count()
        out = call()
        launches[n] = int(_ffi.lib().gdr_launch_count() - c0)
        assert int(out[2].abs().sum()) == 0, f"{name} / {n}: an overflowed list"
    assert not np.isin(out[1].cpu().numpy(), np.nonzero(~live)[0]).any()
    for it in range(warmup + iters):
        for n, call in calls.items():                                # alternating: both see the same clocks and the same cache state
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            b.synchronize()
            if it >= warmup:
                times[n].append(a.elapsed_time(b))
    med = {n: statistics.median(t) for n, t in times.items()}
    return {"case": name, "B": B, "N": N, "d": d, "k": k, "dead_rows": dead, "dtype": "bf16" if bf16 else "fp32", "iters": iters,
            "plain_ms": round(med["plain"], 4), "masked_ms": round(med["masked"], 4),
            "plain_min_ms": round(min(times["plain"]), 4), "masked_min_ms": round(min(times["masked"]), 4),
            "masked_over_plain": round(med["masked"] / med["plain"], 4), "launches_plain": launches["plain"],
            "launches_masked": launches["masked"], "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rows", type=int, default=320_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    lines = []
    D32 = torch.from_numpy(synth.make_corpus(a.rows, 768, seed=1)).to(dev)
    for name, B, bf16 in (("C2 fp32 B=512", 512, False), ("fp32 B=32", 32, False), ("bf16 B=512", 512, True), ("bf16 B=32", 32, True)):
        r = _case(name, B, D32, 100, 1000, bf16, a.iters, a.warmup, dev)
        print(json.dumps(r), flush=True)
        lines.append(json.dumps(r))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
