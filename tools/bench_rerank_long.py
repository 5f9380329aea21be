"""Stage 2 alone (ops.rerank_topk: dot pass + select) over candidate lists on both sides of the 8192-candidate boundary, on one
GPU: queries x beams of 1 x 100, 64 x 10 and 512 x 30 at 1 200 / 8 000 / 10 000 / 40 000 / 200 000 candidates per query, fp32 and
bf16 corpus, seven alphas, k = num beams.  Up to 8192 candidates the one-sort select runs and the chunked form
(chunked=True, GDR_RERANK_CHUNKED) is timed beside it; above, only the chunked form exists.  Times are medians of HIP event
pairs after warm-up.  The CPU baseline is oracle.retrieval_ref.rerank on the same lists, timed on the first --cpu-queries
queries of the batch and reported per query.  Prints one JSON object."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ALPHAS = [0, 0.5, 1, 1.5, 2, 2.5, 3]


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="1x100,64x10,512x30", help="queries x beams, comma separated")
    ap.add_argument("--cands", default="1200,8000,10000,40000,200000", help="candidates per query, comma separated")
    ap.add_argument("--rows", type=int, default=320000, help="corpus rows")
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-queries", type=int, default=1, help="queries of each batch the CPU baseline ranks (0: none)")
    return ap.parse_args(argv)


def event_ms(fn, reps, warm):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in pairs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) for a, b in pairs)
    return {"median_ms": ts[len(ts) // 2], "min_ms": ts[0], "max_ms": ts[-1]}


def main(argv=None):
    args = parse_args(argv)
    import numpy as np
    import torch
    from gdr_amd import ops, synth
    from oracle import retrieval_ref
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    D = synth.make_corpus(args.rows, args.d)
    Dd = {"fp32": torch.from_numpy(D).to(dev)}
    Dd["bf16"] = ops.to_bf16(Dd["fp32"])
    Dt = torch.from_numpy(D)
    rng = np.random.default_rng(7)
    out = {"device": torch.cuda.get_device_name(0), "rows": args.rows, "d": args.d, "alphas": ALPHAS, "results": []}
    for shape in args.shapes.split(","):
        B, R = (int(x) for x in shape.split("x"))
        Q, _ = synth.make_queries(D, B, seed=4)
        Q *= 0.15
        beam = np.sort(rng.standard_normal((B, R)).astype(np.float32) * 2 - 8, axis=1)[:, ::-1].copy()
        Qd, bd = torch.from_numpy(Q).to(dev), torch.from_numpy(beam).to(dev)
        for ncand in (int(x) for x in args.cands.split(",")):
            # R segments of nearly equal length per query (the last takes the remainder), ids drawn over the whole corpus
            lens = np.full(R, ncand // R, np.int64)
            lens[-1] += ncand - lens.sum()
            offs = np.zeros((B, R + 1), np.int32)
            offs[:, 1:] = np.cumsum(lens)
            ids = rng.integers(0, args.rows, (B, ncand), dtype=np.int64).astype(np.int32)
            od, idd = torch.from_numpy(offs).to(dev), torch.from_numpy(ids).to(dev)
            row = {"queries": B, "beams": R, "candidates_per_query": ncand, "k": R}
            for name, corpus in Dd.items():
                run = lambda chunked: ops.rerank_topk(Qd, corpus, od, idd, bd, ALPHAS, R, max_cand=ncand,   # noqa: E731
                                                      cand_stride=ncand, chunked=chunked)
                if ncand <= ops.RERANK_MAX_CAND:
                    row[name + "_one_sort"] = event_ms(lambda: run(False), args.reps, args.warmup)
                    v0, i0 = run(False)
                    v1, i1 = run(True)
                    assert torch.equal(v0, v1) and torch.equal(i0, i1), "the chunked form differs from the one-sort form"
                row[name + "_chunked"] = event_ms(lambda: run(True), args.reps, args.warmup)
            nq = min(B, args.cpu_queries)
            if nq > 0:
                t0 = time.perf_counter()
                retrieval_ref.rerank(torch.from_numpy(Q[:nq]), Dt, [ids[b].tolist() for b in range(nq)], [lens.tolist()] * nq,
                                     beam[:nq].tolist(), ALPHAS, R)
                row["cpu_oracle_ms_per_query"] = (time.perf_counter() - t0) * 1e3 / nq
            out["results"].append(row)
            del od, idd
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
