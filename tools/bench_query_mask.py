"""What a row filter per query costs the corpus search, and where narrow filters begin to overflow:
gdr_sim_topk / gdr_sim_topk_bf16 at config C2's shape (N = 320 000, d = 768, k = 100) as ops.sim_topk issues them —
    plain                 no mask
    live                  live= with 1 000 random dead rows (GDR_SIM_LIVE_MASK: the yardstick)
    allowed_same          allowed= with the same 1 000 rows denied for every query (GDR_SIM_QUERY_MASK)
    allowed_keep_P        allowed= with an independent random filter per query that keeps P % of the rows
all cases ALTERNATING in one process, each call between device events, medians after warm-up.  The flagged times include the
copy of the bitmap(s) into the workspace.  No call repairs an overflowed list (exact_on_overflow=False): `overflowed` is the number
of queries the raw call flags, which ops.sim_topk would re-run exhaustively.  `copy_ms` times the B x M-byte strided bitmap copy
alone.  Prints one JSON line per case and, with --out, writes them to a file.

    python tools/bench_query_mask.py --out profiles/query_mask.jsonl"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gdr_amd import _ffi, ops, synth  # noqa: E402


def _timed(call):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = call()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def _config(name, B, D32, k, dead, keeps, bf16, iters, warmup, dev):
    N, d = D32.shape
    Q = torch.from_numpy(synth.make_queries(D32[:4096].cpu().numpy(), B, seed=2)[0]).to(dev)
    D = D32
    if bf16:
        D, Q = ops.to_bf16(D32), ops.to_bf16(Q)
    gone = np.random.default_rng(3).choice(N, dead, replace=False)
    live = np.ones(N, bool)
    live[gone] = False
    live_d = torch.from_numpy(live).to(dev)
    L = ops.LiveRows.from_bool(live_d)
    ws = ops.Workspace(dev)
    run = lambda **kw: ops.sim_topk(Q, D, k, workspace=ws, exact_on_overflow=False, return_status=True, **kw)   # noqa: E731
    filters = {"allowed_same": ops.QueryRows.from_bool(live_d.expand(B, N))}
    gen = torch.Generator(device=dev).manual_seed(5)
    for keep in keeps:
        filters[f"allowed_keep_{round(keep * 100)}"] = ops.QueryRows.from_bool(torch.rand((B, N), device=dev, generator=gen) < keep)
    calls = {"plain": lambda: run(), "live": lambda: run(live=L)}
    for n, R in filters.items():
        calls[n] = lambda R=R: run(allowed=R)
    launches, overflowed = {}, {}
    for n, call in calls.items():
        c0 = _ffi.lib().gdr_launch_count()
        out = call()
        launches[n] = int(_ffi.lib().gdr_launch_count() - c0)
        overflowed[n] = int((out[2] != 0).sum())
        if n in ("live", "allowed_same"):
            assert overflowed[n] == 0 and not np.isin(out[1].cpu().numpy(), gone).any()
    # the bitmap copy alone, into the head of a buffer laid out as the workspace is
    words = filters["allowed_same"].words
    M = (4 * words.shape[1] + 255) // 256 * 256
    buf = torch.empty(B * M, dtype=torch.uint8, device=dev)
    slots = buf.view(torch.int32).view(B, M // 4)[:, :words.shape[1]]
    times = {n: [] for n in calls}
    copy = []
    for it in range(warmup + iters):
        for n, call in calls.items():                                # alternating: all see the same clocks and the same cache state
            t, _ = _timed(call)
            if it >= warmup:
                times[n].append(t)
        t, _ = _timed(lambda: slots.copy_(words))
        if it >= warmup:
            copy.append(t)
    copy_ms = statistics.median(copy)
    base = {"config": name, "B": B, "N": N, "d": d, "k": k, "dtype": "bf16" if bf16 else "fp32", "iters": iters,
            "bitmap_bytes": B * M, "copy_ms": round(copy_ms, 4), "copy_GBps": round(2 * B * words.shape[1] * 4 / copy_ms / 1e6, 1),
            "device": torch.cuda.get_device_name(0)}
    rows = []
    for n in calls:
        med = statistics.median(times[n])
        rows.append(dict(base, case=n, ms=round(med, 4), min_ms=round(min(times[n]), 4), launches=launches[n], overflowed=overflowed[n],
                         over_plain=round(med / statistics.median(times["plain"]), 4),
                         minus_live_ms=round(med - statistics.median(times["live"]), 4)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rows", type=int, default=320_000)
    ap.add_argument("--keep", default="0.9,0.5,0.3,0.25,0.2,0.15,0.1", help="fractions of the rows the random per-query filters keep")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    keeps = [float(x) for x in a.keep.split(",")]
    lines = []
    D32 = torch.from_numpy(synth.make_corpus(a.rows, 768, seed=1)).to(dev)
    for name, B, bf16 in (("C2 fp32 B=512", 512, False), ("fp32 B=32", 32, False), ("bf16 B=512", 512, True), ("bf16 B=32", 32, True)):
        for r in _config(name, B, D32, 100, 1000, keeps, bf16, a.iters, a.warmup, dev):
            print(json.dumps(r), flush=True)
            lines.append(json.dumps(r))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
