"""Where the gather mode beats the dense masked search: gdr_sim_topk / gdr_sim_topk_bf16 at config C2's shape
(N = 320 000, d = 768, k = 100), 512 and 32 queries, independent random filters that keep exactly R rows per query —
    dense     ops.sim_topk(allowed=, gather=False): the dense masked call, the status read-back and the exhaustive re-run of the
              queries it flags — what the call did before the gather mode existed
    gather    ops.sim_topk(allowed=, gather=R, exact_on_overflow=False): GDR_SIM_ROW_GATHER at ceil(R / 4096) chunks, no read-back
    auto      ops.sim_topk(allowed=, gather="auto"): the routed call, with its read-back of the counts
and the skewed batch (one query that allows 8 000 rows beside B - 1 that allow 300) beside the two uniform ones.  All cases
ALTERNATING in one process, each call between device events, medians after warm-up; the times include the copy of the bitmaps into
the workspace.  gather_TBps = sum of n_q x d x element size / gather time: the achieved row-read rate.  Prints one JSON line per case
and, with --out, writes them to a file.

    python tools/bench_query_gather.py --out profiles/query_gather.jsonl"""
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


def _exactly(B, N, counts, dev, gen):
    """QueryRows whose query q allows exactly counts[q] uniformly drawn rows."""
    R = ops.QueryRows(B, N, dev)
    for lo in range(0, B, 32):
        r = torch.rand((min(32, B - lo), N), device=dev, generator=gen, dtype=torch.float64)   # 53 bits: no two draws of a row tie
        thr = torch.stack([r[j].kthvalue(int(counts[lo + j])).values for j in range(r.shape[0])])
        R._words[lo:lo + 32] = ops.QueryRows.from_bool(r <= thr[:, None])._words
    assert R.counts().tolist() == [int(c) for c in counts]
    return R


def _config(name, B, D32, k, kept, bf16, iters, warmup, dev):
    N, d = D32.shape
    Q = torch.from_numpy(synth.make_queries(D32[:4096].cpu().numpy(), B, seed=2)[0]).to(dev)
    D = D32
    if bf16:
        D, Q = ops.to_bf16(D32), ops.to_bf16(Q)
    esz = 2 if bf16 else 4
    ws = ops.Workspace(dev)
    gen = torch.Generator(device=dev).manual_seed(5)
    cases = {f"keep_{r}": [r] * B for r in kept}
    cases["skew_8000_beside_300"] = [8000] + [300] * (B - 1)
    cases["uniform_300_at_2_chunks"] = [300] * B
    cases["uniform_8000"] = [8000] * B
    calls, meta = {}, {}
    for n, counts in cases.items():
        R = _exactly(B, N, counts, dev, gen)
        cap = 8192 if n.startswith(("skew", "uniform")) else max(counts)
        calls[n, "gather"] = lambda R=R, cap=cap: ops.sim_topk(Q, D, k, workspace=ws, allowed=R, gather=cap, exact_on_overflow=False, return_status=True)
        if n.startswith("keep"):
            calls[n, "dense"] = lambda R=R: ops.sim_topk(Q, D, k, workspace=ws, allowed=R, gather=False, return_status=True)
            calls[n, "auto"] = lambda R=R: ops.sim_topk(Q, D, k, workspace=ws, allowed=R, gather="auto", return_status=True)
        raw = ops.sim_topk(Q, D, k, workspace=ws, allowed=R, exact_on_overflow=False, return_status=True)
        c0 = _ffi.lib().gdr_launch_count()
        gv, gi, gst = calls[n, "gather"]()
        meta[n] = {"rows": sum(counts), "chunks": ops.gather_chunks(cap), "gather_launches": int(_ffi.lib().gdr_launch_count() - c0),
                   "dense_overflowed": int((raw[2] != 0).sum())}
        assert int(gst.abs().sum()) == 0
        if (n, "dense") in calls:                                    # the two routes return the same documents
            dv, di, _ = calls[n, "dense"]()
            meta[n]["ids_equal_dense"] = round(float((di == gi).float().mean()), 6)
            assert torch.allclose(dv, gv, rtol=1e-3 if bf16 else 1e-4, atol=1e-3 if bf16 else 1e-4)
    times = {key: [] for key in calls}
    for it in range(warmup + iters):
        for key, call in calls.items():                              # alternating: all see the same clocks and the same cache state
            t, _ = _timed(call)
            if it >= warmup:
                times[key].append(t)
    base = {"config": name, "B": B, "N": N, "d": d, "k": k, "dtype": "bf16" if bf16 else "fp32", "iters": iters, "device": torch.cuda.get_device_name(0)}
    rows = []
    for n in cases:
        g = statistics.median(times[n, "gather"])
        row = dict(base, case=n, gather_ms=round(g, 4), gather_min_ms=round(min(times[n, "gather"]), 4),
                   gather_TBps=round(meta[n]["rows"] * d * esz / g / 1e9, 3), **meta[n])
        if (n, "dense") in times:
            dn = statistics.median(times[n, "dense"])
            row.update(dense_ms=round(dn, 4), dense_min_ms=round(min(times[n, "dense"]), 4), auto_ms=round(statistics.median(times[n, "auto"]), 4),
                       dense_over_gather=round(dn / g, 3))
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rows", type=int, default=320_000)
    ap.add_argument("--keep", default="320,1000,3200,8192,16384,32768,65536", help="rows the random per-query filters keep")
    ap.add_argument("--configs", default="fp32:512,fp32:32,bf16:512,bf16:32")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    kept = [int(x) for x in a.keep.split(",")]
    lines = []
    D32 = torch.from_numpy(synth.make_corpus(a.rows, 768, seed=1)).to(dev)
    for cfg in a.configs.split(","):
        dt, B = cfg.split(":")
        for r in _config(f"{dt} B={B}", int(B), D32, 100, kept, dt == "bf16", a.iters, a.warmup, dev):
            print(json.dumps(r), flush=True)
            lines.append(json.dumps(r))
            if a.out:
                with open(a.out, "w") as f:
                    f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
