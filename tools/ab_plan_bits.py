"""Every entry point that reaches a kernel built on csrc/scan.h (the one-workgroup scans, the wave scans of the place kernels, the
bitmap words), an integer wave sum of csrc/common.h or the ordered row sum of the centroids, on fixed synthetic inputs, for comparing
two builds of libgdr_hip.so bit for bit on one GPU — one process per library, the Python files being the same:

    GDR_HIP_LIB=/path/to/parent/libgdr_hip.so timeout -k 10 600 python tools/ab_plan_bits.py --out parent.json \
        && timeout -k 10 600 python tools/ab_plan_bits.py --out head.json \
        && python tools/ab_plan_bits.py --compare parent.json head.json

A run records, per call, the sha256 of all output bytes and the library's launch count (gdr_launch_count); --compare (no GPU) prints the
calls whose digest or count differ and exits 1 if there is one.  Under `rocprofv3 --kernel-trace --stats -- python tools/ab_plan_bits.py
--out x.json --repeat 10` the same run gives the per-launch times of those kernels (tools/trace_kernel_ab.py --only); --repeat makes
every call that often, so that a kernel of two launches has twenty to take a mean over (the digest is the last call's).

The shapes are the small ones of the tests (tests/batch_rounds.py and the files it names), on both sides of every boundary of a scan:
1023 / 1024 / 1025 entries of a round, ceil(n / 1024) = 1 / 2 / 3 consecutive entries per thread, 256 / 257 / 300 beam rows."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from ab_attention_bits import compare  # noqa: E402  (the same record format)

LIFE_SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 5000)   # tests/test_gpu_lifecycle.py: nine clusters


def run(out_path, repeat=1):
    import torch
    import batch_rounds as BR
    import sim_widths
    from gdr_amd import _ffi, codec, ops, synth
    from gdr_amd.modeling import GDRModel
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    count = _ffi.lib().gdr_launch_count
    out = {}

    def call(name, fn):
        n0 = count()
        for _ in range(repeat):
            res = fn()
        res = res if isinstance(res, (tuple, list)) else (res,)
        h = hashlib.sha256()
        for t in res:
            if t is None:
                continue
            t = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
            h.update(np.ascontiguousarray(t).tobytes())
        torch.cuda.synchronize()
        out[name] = [h.hexdigest(), int(count() - n0) // repeat]
        return res

    def d(a, dtype=None):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)

    # ---- pack_len / pack_scan: the packed forwards of both towers, one partial round, exactly one, two
    t5 = ops.T5EncoderHandle(BR.t5_config(), BR.t5_state_dict(), dev)
    bert = ops.BertEncoderHandle(BR.bert_cfg(), BR.bert_state_dict(), dev)
    for B in (1023, 1024, 1025):
        for tag, enc, vocab in (("t5", t5, BR.t5_config().vocab_size), ("bert", bert, BR.bert_cfg()["vocab_size"])):
            ids, mask = BR.tower_tokens(B, BR.TOWER_L, vocab)
            it, mt = d(np.array(ids)), d(np.array(mask))
            call(f"pack/{tag}/B{B}/hidden+pooled", lambda: enc.forward(it, mt, ragged=True, live_rows_hint=int(BR.kept(mask).sum())))
            call(f"pack/{tag}/B{B}/pooled-only", lambda: enc.forward(it, mt, ragged=True, want_hidden=False))
    del t5, bert

    # ---- rows_count / rows_units / rows_place: the gather top-k, one round of queries and two
    for B in (1024, 1025):
        s = BR.gather_case(B, False)
        R = ops.QueryRows.from_bool(d(np.array(s.allowed)))
        Qd, Dd = s.Qt.to(dev), s.Dt.to(dev)
        call(f"gather/B{B}", lambda: ops.sim_topk(Qd, Dd, BR.GATHER_K, allowed=R, gather=BR.GATHER_CAP, exact_on_overflow=False,
                                                   return_status=True))

    # ---- compact_count / compact_scan / compact_place: one scan step of 1024 tiles of 4096 rows, and one row more
    for N in (1024 * 4096, 1024 * 4096 + 1):
        live = np.random.default_rng(N).random(N) >= 0.3
        plan = call(f"compact_plan/N{N}", lambda: (lambda p: (p.new_id, p.old_id))(ops.compact_plan(ops.LiveRows.from_bool(d(live)))))
        del plan

    # ---- insert_scan (and remove_count): insert and removal at 9 clusters (per = 1) and at 2049 (per = 3)
    rng = np.random.default_rng(17)
    offs9 = np.concatenate([[0], np.cumsum(LIFE_SIZES)]).astype(np.int32)
    mem9 = rng.permutation(8000)[:offs9[-1]].astype(np.int32)
    new9 = np.arange(8000, 8300, dtype=np.int32)
    offs, mem, new_ids, targets = BR.insert_case()
    _, _, gone = BR.remove_case()
    for tag, o, m, n, t, g in (("C9", offs9, mem9, new9, rng.integers(0, 9, 300), np.unique(rng.choice(8000, 3000, replace=False))),
                               ("C2049", offs, mem, new_ids, targets, gone)):
        call(f"cluster_insert/{tag}", lambda: ops.cluster_insert(d(o, np.int32), d(m, np.int32), d(n, np.int32), d(t, np.int32)))
        call(f"cluster_remove/{tag}", lambda: ops.cluster_remove(d(o, np.int32), d(m, np.int32), d(g, np.int32)))

    # ---- centroid_kernel, part_scan, cent_chunk: ordered row sums and the partition's scan at 1024 / 1025 / 1023 entries
    X = (rng.standard_normal((8000, 96)) * rng.uniform(0.5, 4.0, (8000, 1))).astype(np.float32)
    Xd = d(X)
    seg = np.concatenate([np.sort(mem9[offs9[c]:offs9[c + 1]]) for c in range(9)]).astype(np.int32)
    call("cluster_centroids/C9", lambda: ops.cluster_centroids_csr(Xd, d(offs9), d(seg)))
    for k, sizes in ((30, (7000, 1, 255, 256, 257, 31)),) + BR.PARTITION_CASES:
        o = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
        rows = np.concatenate([np.sort(rng.choice(8000, s, replace=False)) for s in sizes]).astype(np.int32)
        lab = rng.integers(0, k, rows.size).astype(np.int32)
        res = call(f"kmeans_partition/k{k}/m{BR.partition_scan_entries(k, sizes)}", lambda: ops.kmeans_partition(d(rows), d(lab), d(o), k))
        call(f"kmeans_centroids/k{k}/m{BR.partition_scan_entries(k, sizes)}", lambda: ops.kmeans_centroids(Xd, res[1], res[0]))

    # ---- prefix_plan: generate() with a prefix table at 171 x 6 = 1026 beam rows (two rows per thread)
    cfg, B, R = BR.prefix_config(), 171, BR.PREFIX_R
    ids, mask = BR.prefix_tokens(B)
    model = GDRModel(cfg, BR.prefix_state_dict(), dev, prefix_trie=BR.prefix_trie(3))
    call("generate/prefix-table/rows1026", lambda: (lambda r: (r[0][0], np.array(r[0][1], np.float32)))(
        model.generate(d(ids), attention_mask=d(mask), max_length=cfg.max_output_length, num_beams=R, length_penalty=0.8,
                       num_return_sequences=R, output_scores=True)))
    del model

    # ---- cluster_candidates: one round of 256 beam rows, a second of one row, a second of 44
    V, ml = 30, 10
    names, _, coffs, _ = synth.make_cluster_ids(600, cluster_size=3, V=V)
    index = codec.ClusterIndex(names, coffs, np.random.Generator(np.random.PCG64(5)).permutation(600).astype(np.int32))
    dci = ops.DeviceClusterIndex(index, dev, V)
    for R in (256, 257, 300):
        g = np.random.Generator(np.random.PCG64(R))
        rows = np.zeros((2 * R, ml), np.int64)
        for r in range(2 * R):
            if r % 37 != 5:                                   # the others stay START, PAD...: rows that name no cluster
                toks = codec.encode_single_newid(names[int(g.integers(0, len(names)))], kary=V)
                rows[r, 1:1 + len(toks)] = toks
        def blocks():                                         # a block past its last offset is not written: not compared
            cl, offs, ids, _ = dci.candidates(d(rows), 2, R)
            return (cl, offs) + tuple(ids[b, :int(offs[b, R])] for b in range(2))
        call(f"cluster_candidates/R{R}", blocks)

    # ---- sim_live_thr_fixup: fewer than k live rows in the sample tiles, one bitmap for all queries and one per query
    N, dim, k, B = 25000, 64, 10, 4
    stride = sim_widths.plan(N, k)[0]
    assert stride > 1
    D = synth.make_corpus(N, dim, seed=N + dim)
    Q, _ = synth.make_queries(D, B, seed=3)
    live = ~sim_widths.in_sample_tile(N, stride)
    live[np.nonzero(~live)[0][:5]] = True
    live[N - 3:] = False                                       # the last word has dead bits below N as well
    Qd, Dd = d(Q), d(D)
    L = ops.LiveRows.from_bool(d(live))
    # the raw call: thr = -inf keeps every row, the lists overflow and their content depends on the order of arrival — the status (1 for
    # every query the fix-up reached) is what is compared; then the call that re-runs the flagged queries exhaustively, whole
    call("sim_topk/live-mask/short-sample/status", lambda: ops.sim_topk(Qd, Dd, k, live=L, exact_on_overflow=False, return_status=True)[2])
    call("sim_topk/live-mask/short-sample", lambda: ops.sim_topk(Qd, Dd, k, live=L, return_status=True))
    allowed = np.tile(live, (B, 1))
    allowed[1] = True
    allowed[2] = False
    allowed[2, 100:107] = True                                 # fewer than k rows in all: a list that ends in -inf / -1
    A = ops.QueryRows.from_bool(d(allowed))
    call("sim_topk/query-mask/short-sample/status", lambda: ops.sim_topk(Qd, Dd, k, allowed=A, exact_on_overflow=False, return_status=True)[2])
    call("sim_topk/query-mask/short-sample", lambda: ops.sim_topk(Qd, Dd, k, allowed=A, return_status=True))

    with open(out_path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
    print(f"{len(out)} calls, {sum(v[1] for v in out.values())} kernel launches -> {out_path}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--repeat", type=int, default=1)
    ap.add_argument("--compare", nargs=2)
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    run(args.out, args.repeat)
