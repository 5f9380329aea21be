"""What the masked pre-filter buys a filtered corpus search: gdr_sim_topk_prefilter_masked against the call the same
request takes without it, at config C2's shape (N = 320 000, d = 768, k = 100) for 512 and 32 queries —
    fp32_<form>           ops.sim_topk(Q, D, k, live= / allowed=)                               (gdr_sim_topk with the mask: the parent path)
    prefilter_<form>      ops.sim_topk(Q, PrefilteredCorpus(D, masks=True), k, live= / allowed=) (gdr_sim_topk_prefilter_masked)
with <form> = live_F (one bitmap, a random fraction F of the rows live) and query_F (independent random rows per query), F = 1.0, 0.99,
0.9, 0.5; and the yardstick, the two UNMASKED calls (fp32_plain, prefilter_plain) at the same B.  All calls ALTERNATE in one process, each
between device events, medians after warm-up; the times include the copy of the bitmap(s) into the workspace.  No call repairs a
flagged list (exact_on_overflow=False): `flagged` is the number of queries the raw call flags.  `parent_spread_ms` is the parent
path's own run-to-run spread — the medians of the odd and of the even rounds of the SAME fp32 call, apart — the scale against which
`gain_ms` (fp32 median minus pre-filter median) is to be read.  Prints one JSON line per pair and, with --out, writes them to a file.

    python tools/bench_prefilter_mask.py --out profiles/prefilter_mask.jsonl"""
import argparse
import json
import os
import statistics
import sys

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


def _config(B, D, P, k, fractions, iters, warmup, dev):
    N, d = D.shape
    Q = torch.from_numpy(synth.make_queries(D[:4096].cpu().numpy(), B, seed=2)[0]).to(dev)
    ws = ops.Workspace(dev)
    run = lambda corpus, **kw: ops.sim_topk(Q, corpus, k, workspace=ws, exact_on_overflow=False, return_status=True, **kw)   # noqa: E731
    gen = torch.Generator(device=dev).manual_seed(5)
    pairs = {"plain": {}}
    for f in fractions:
        live = torch.rand(N, device=dev, generator=gen) < f if f < 1.0 else torch.ones(N, dtype=torch.bool, device=dev)
        pairs[f"live_{f}"] = {"live": ops.LiveRows.from_bool(live)}
        allowed = torch.rand((B, N), device=dev, generator=gen) < f if f < 1.0 else torch.ones((B, N), dtype=torch.bool, device=dev)
        pairs[f"query_{f}"] = {"allowed": ops.QueryRows.from_bool(allowed)}
        del allowed
    calls = {}
    for form, kw in pairs.items():
        calls[f"fp32_{form}"] = lambda kw=kw: run(D, **kw)
        calls[f"prefilter_{form}"] = lambda kw=kw: run(P, **kw)
    launches, flagged = {}, {}
    for n, call in calls.items():
        c0 = _ffi.lib().gdr_launch_count()
        out = call()
        launches[n] = int(_ffi.lib().gdr_launch_count() - c0)
        flagged[n] = int((out[2] != 0).sum())
    same = {}
    for form in pairs:                                               # the two paths return the same documents wherever neither flags
        a, b = calls[f"fp32_{form}"](), calls[f"prefilter_{form}"]()     # (rows that differ: ties within fp32 summation noise)
        ok = (a[2] == 0) & (b[2] == 0)
        same[form] = round((a[1][ok] == b[1][ok]).all(dim=1).float().mean().item(), 4) if bool(ok.any()) else None
    times = {n: [] for n in calls}
    for it in range(warmup + iters):
        for n, call in calls.items():                                # alternating: all see the same clocks and the same cache state
            t, _ = _timed(call)
            if it >= warmup:
                times[n].append(t)
    med = {n: statistics.median(t) for n, t in times.items()}
    yard = med["fp32_plain"] - med["prefilter_plain"]
    rows = []
    for form in pairs:
        fp, pre = f"fp32_{form}", f"prefilter_{form}"
        spread = abs(statistics.median(times[fp][0::2]) - statistics.median(times[fp][1::2]))
        rows.append({"B": B, "N": N, "d": d, "k": k, "form": form, "iters": iters, "fp32_ms": round(med[fp], 4),
                     "prefilter_ms": round(med[pre], 4), "fp32_min_ms": round(min(times[fp]), 4), "prefilter_min_ms": round(min(times[pre]), 4),
                     "gain_ms": round(med[fp] - med[pre], 4), "parent_spread_ms": round(spread, 4),
                     "fp32_over_prefilter": round(med[fp] / med[pre], 4), "unmasked_gain_ms": round(yard, 4),
                     "fp32_flagged": flagged[fp], "prefilter_flagged": flagged[pre], "fp32_launches": launches[fp],
                     "prefilter_launches": launches[pre], "rows_with_identical_ids": same[form], "device": torch.cuda.get_device_name(0)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rows", type=int, default=320_000)
    ap.add_argument("--batches", default="512,32")
    ap.add_argument("--live", default="1.0,0.99,0.9,0.5", help="fractions of the rows that stay live / allowed")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    D = torch.from_numpy(synth.make_corpus(a.rows, 768, seed=1)).to(dev)
    P = ops.PrefilteredCorpus(D, masks=True)
    lines = []
    for B in (int(x) for x in a.batches.split(",")):
        for r in _config(B, D, P, 100, [float(x) for x in a.live.split(",")], a.iters, a.warmup, dev):
            print(json.dumps(r), flush=True)
            lines.append(json.dumps(r))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
