#!/usr/bin/env python3
"""bench.py — queries/sec of GDR's dense-retrieval hot path on MI355X (BASELINE.json metric).

A step = one pass of the hot path over one batch of synthetic input:
    T5-base encoder forward on `batch` tokenised queries (int64[batch,40])  ->  CLS pool  ->
    fused Q·Dᵀ + top-100 over the resident 320 000 x 768 fp32 corpus.
N = 1 runs BASELINE config C2 (batch 512, whole corpus on one GPU).  N > 1 (one process per GPU, launched by
torch.distributed.run) runs C4's layout with weak scaling: every rank encodes its own 512 queries, the corpus
is row-sharded N ways, pooled queries are all-gathered, each rank searches its shard for all 512·N queries,
and ONE all-to-all of the packed per-shard (score,id,status)[B,k+1] lists hands every rank the lists of its own 512
queries, which it merges (gdr_amd/dist.py); the exchange runs on a side stream under the next step's encoder
(--replicated-merge: one all-gather + merge of all queries on every rank, no overlap).

The encoder runs in its ragged form by default (PAD token rows are not computed, the last block runs on the CLS rows
only; pooled output bit-identical to the padded form — tests/test_gpu_ragged.py); --encoder padded computes all rows.

`python bench.py --gpus N` needs no launcher typed by hand: with no RANK in the environment the command (which has not
touched a GPU) starts the N ranks as fresh child processes of `python -m torch.distributed.run` (gdr_amd/launch.py), relays
rank 0's JSON line and exits non-zero if any rank does; under torch.distributed.run it is a rank.

--workload c3 / c5 measure the TWO-STAGE path (BASELINE configs C3 / C5) in the same JSON contract: a step = one batch of
queries per GPU through GDRRetriever.validation_step_i — encoder -> docid beam decode -> device cluster lookup -> in-cluster
rerank over 7 alphas -> host formatting; at N > 1 the corpus is row-sharded and stage 2 is dist.ShardedIndex.rerank_own
(one all-gather of queries + candidate blocks, per-shard scoring, one all-to-all, merge).  c3: 320k x 768 fp32, beam 10,
64 queries per GPU; c5: 1M x 768 bf16 corpus, beam 30, bf16 linear operands, 512 queries per GPU (4 096 at 8 GPUs).

Prints ONE JSON line (rank 0).  `roofline` is for the dominant kernel, the fp32 MFMA GEMM that serves every
encoder linear: algorithmic flops per launch / average launch duration, both measured live over the timed
region with hipEvent pairs recorded by the library on the launch stream (gdr_prof_*).

A plain run sets up, warms up, times --steps steps, writes the last step's outputs (--dump-outputs DIR) and prints the
line.  Everything else is behind --full (then the `#stages` line and bench_stages.json come first): `cpu_baseline`, the
oracle ("port" of the reference's CPU path) timed on this box's host cores on a bounded sample; `recall` / `parity`
against the oracle; the same step in its other forms (other similarity form, padded encoder, exploratory split forms);
for c3 / c5 the profiled replay behind `roofline`; and `stages` (N = 1, measured AFTER the headline timed region, never
part of `value`), the other stages of the path: latency-mode similarity against the HBM roof, generate() at the C3 and
infer.sh settings against their flop / weight-byte floors, the two-stage C3 / C5 rates and the bf16 precision mode.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

F32_MFMA_PEAK_TFLOPS = 157.3      # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, dense
BF16_MFMA_PEAK_TFLOPS = 2500.0    # dense bf16 MFMA (no sparsity)
HBM_PEAK_GBS = 8000.0
LINE_LIMIT = 4096                 # the round driver keeps the last 8 KB of stdout: the headline line must fit with room to spare


def sig(x, n=5):
    """Every float of a JSON-able object rounded to n significant digits (the line is read by people and by the driver)."""
    if isinstance(x, float):
        return float(f"{x:.{n}g}") if x == x and abs(x) != float("inf") else None
    if isinstance(x, dict):
        return {k: sig(v, n) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [sig(v, n) for v in x]
    return x


TAIL_BUDGET = 7600               # both lines together must fit the driver's 8 KB stdout tail: then the tail starts at the '#'


def compact(x, drop=("note", "sample", "cpu_model", "recall_rule", "config_note", "roofline_note", "roofline_sampling")):
    """The stdout form of the detail object: prose keys dropped (they stay in bench_stages.json), floats to 4 digits."""
    if isinstance(x, dict):
        return {k: compact(v, drop) for k, v in x.items() if not (k in drop or k.endswith("_note"))}
    if isinstance(x, (list, tuple)):
        return [compact(v, drop) for v in x]
    return sig(x, 4) if isinstance(x, float) else x


def emit(result, detail=None):
    """Rank 0's output: the detail object on a `#stages` line (in full, with its prose, in bench_stages.json next to this script), then
    THE one JSON line — headline, roofline, cpu_baseline, recall / parity and a dozen-odd stage scalars — which must stay under
    LINE_LIMIT.  The two lines together stay under TAIL_BUDGET: the driver keeps the last 8 KB of stdout, and a tail that starts inside
    the `#stages` line could begin with a `{` of its own."""
    line = json.dumps(sig(result))
    if len(line) > LINE_LIMIT:
        raise SystemExit(f"bench: the JSON line is {len(line)} bytes (> {LINE_LIMIT}): move detail to the #stages line")
    if detail:
        try:
            with open(os.path.join(REPO, "bench_stages.json"), "w") as f:
                f.write(json.dumps(sig(detail)) + "\n")
        except OSError:
            pass
        small = compact(detail)
        text = json.dumps(small)
        # still too long: drop the least consulted stage objects one by one (they remain in the file)
        order = ("rerank", "prefix_table", "generate_trie_constrained", "c3_two_stage_B512", "kernels", "doc_tower_bert_base_L128",
                 "c5_two_stage", "c2_step_split_bf16", "similarity_topk_f32_prefilter", "c2_step_padded", "c2_step_all_fp32",
                 "c2_step_bf16_prefilter", "bf16_mode_generate_B64_beam30", "bf16_mode_c2_step", "c3_two_stage_infer_sh", "c3_best_sustained")
        for key in order:
            if len(text) + len(line) + 10 <= TAIL_BUDGET:
                break
            st_ = small.get("stages") or {}
            if isinstance(st_.get(key), dict) and "parity" in st_[key]:     # first the nested oracle-check object, then the stage itself
                st_[key].pop("parity", None)
                text = json.dumps(small)
                if len(text) + len(line) + 10 <= TAIL_BUDGET:
                    break
            st_.pop(key, None)
            small.pop(key, None)
            text = json.dumps(small)
        print("#stages " + text)
    print(line)
    sys.stdout.flush()


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(path, arrays):
    """--dump-outputs: every array as path/<name>.npy, float32 if it is a float of 32 bits or fewer, float64 otherwise (ids are
    exact in float64).  All arrays share their leading (query) axis; if together they exceed DUMP_LIMIT_BYTES, the same fixed,
    seeded sample of queries is taken from each and its query numbers go to path/rows.npy."""
    out = {}
    for name, x in arrays.items():
        if isinstance(x, torch.Tensor):
            x = x.detach()
            x = (x.float() if x.is_floating_point() and x.element_size() <= 4 else x.double()).cpu().numpy()
        x = np.asarray(x)
        out[name] = x.astype(np.float32 if x.dtype.kind == "f" and x.dtype.itemsize <= 4 else np.float64)
    n = {x.shape[0] for x in out.values()}
    assert len(n) == 1, f"dump_outputs: leading axes differ {n}"
    n = n.pop()
    total = sum(x.nbytes for x in out.values())
    if total + 128 * len(out) > DUMP_LIMIT_BYTES:         # 128: an .npy header
        per_row = total / n + 8                           # + its entry in rows.npy
        rows = np.sort(np.random.default_rng(0).choice(n, int((DUMP_LIMIT_BYTES - 4096) // per_row), replace=False))
        out = {name: x[rows] for name, x in out.items()}
        out["rows"] = rows.astype(np.float64)
    os.makedirs(path, exist_ok=True)
    for name, x in out.items():
        np.save(os.path.join(path, name + ".npy"), x)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", choices=["c2", "c3", "c5"], default="c2",
                    help="c2 (default, the headline): encoder + Q.D^T top-100; c3 / c5: the two-stage GDR path (beam decode "
                         "-> in-cluster rerank), c5 with the 1M-row bf16 corpus, beam 30 and bf16 linear operands")
    ap.add_argument("--batch", type=int, default=None, help="queries per GPU per step (default: 512 for c2 / c5, 64 for c3)")
    ap.add_argument("--corpus", type=int, default=None, help="corpus rows (default: 320000; c5: 1000000)")
    ap.add_argument("--beams", type=int, default=None, help="c3 / c5: num_beams = num_return_sequences (default 10 / 30)")
    ap.add_argument("--depth", type=int, default=2, help="c3 / c5: batches in flight (GDRRetriever.validation_steps)")
    ap.add_argument("--constrained", action="store_true",
                    help="c3 / c5: constrain the beams to the corpus' docid trie (generation_utils_previous.py:714-729) — every "
                         "hypothesis names a real cluster and the call leaves its step loop early, as a trained model does")
    ap.add_argument("--backend", choices=["nccl", "gloo"], default="nccl",
                    help="torch.distributed backend of the ranks: nccl (= RCCL over xGMI, the product path) or gloo (collectives staged "
                         "through the host: lets N ranks share ONE GPU, which RCCL refuses — used by the tests to run the N > 1 code "
                         "path with real compute on a one-GPU box; its numbers are not a scaling measurement)")
    ap.add_argument("--launcher", action="store_true",
                    help="start the rank processes through torch.distributed.run even for --gpus 1 (a 1-rank RCCL group)")
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--dtype", choices=["f32", "bf16"], default="f32",
                    help="f32 = the reference's precision (the headline); bf16 = config C5's precision mode: bf16 linear "
                         "operands in the encoder and a bf16 corpus, fp32 accumulate (not comparable with the f32 line)")
    ap.add_argument("--encoder", choices=["ragged", "padded"], default="ragged",
                    help="ragged (default): PAD token rows are not computed and only the CLS rows go through the last "
                         "block (exact: pooled output bit-identical to the padded form); padded: every one of the "
                         "batch x 40 rows through all 48 linears, as the reference does")
    ap.add_argument("--encoder-form", choices=["f32", "f16x2", "bf16x3", "bf16x3-16"], default="f32",
                    help="c2, --dtype f32 only.  f32 (default, the headline): strict-fp32 MFMA linears.  EXPLORATORY forms beside it (r06): the "
                         "encoder's fp32 linears carried through 16-bit MFMAs as planes, fp32 accumulate — f16x2: fp16 hi + fp16 (x - hi) * 2^11, "
                         "22 bits, three blocks (GEMM error against float64 below the fp32 MFMA kernel's); bf16x3: 24 bits, six blocks; "
                         "bf16x3-16: the first three bf16 blocks, 16 bits (narrower than fp32).  The line says so: workload tag, dtype, and the "
                         "roofline prices the 16-bit MFMA work against the bf16 matrix peak")
    ap.add_argument("--replicated-merge", action="store_true",
                    help="N > 1: all-gather the per-shard lists and merge all queries on every rank (instead of the "
                         "all-to-all that hands each rank the lists of its own queries)")
    ap.add_argument("--sim-prefilter", choices=["off", "bf16"], default="bf16",
                    help="c2: bf16 (default since r06, accepted by the r05 verdict #7) = gdr_sim_topk_prefilter: the corpus-wide pass on the "
                         "bf16 MFMA path over a bf16 image of the corpus (+50 %% corpus memory), exact fp32 rescoring of the few hundred docs per "
                         "query inside the proven error band — the top-k of the FP32 scores for every input (tests/test_gpu_prefilter.py), "
                         "workload tagged /prefilter, the all-fp32 step timed beside it (`all_fp32`); off = the all-fp32 corpus pass")
    ap.add_argument("--prof-every", type=int, default=4,
                    help="c2: the library brackets every dense launch of every N-th step of the timed region with a hipEvent pair (the "
                         "roofline's per-launch durations); 1 = every step.  Two event packets per launch are not free: around every "
                         "launch of every step they cost 2.4 %% of the step's throughput")
    ap.add_argument("--full", action="store_true",
                    help="also run what the headline does not need: CPU baseline, recall / parity against the oracle, the other "
                         "forms of the step, the c3 / c5 profiled replay and the stages (the --no-* options below select among them)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the timed path returned in its last step as DIR/<name>.npy "
                         "(float32 / float64; ids as float64; at most 64 MB in all, else the same seeded sample of rows of each)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-recall", action="store_true")
    ap.add_argument("--no-parity", action="store_true", help="c3 / c5: skip the oracle check of the step's output")
    ap.add_argument("--parity-queries", type=int, nargs=2, default=None, metavar=("STAGE1", "STAGE2"),
                    help="c3 / c5: queries of the step held against the oracle in stage 1 (beam decode; default 4, 2 above beam 10) "
                         "and stage 2 (rerank; default 64)")
    ap.add_argument("--no-stages", action="store_true", help="skip the stages (other stages of the path, N = 1)")
    ap.add_argument("--no-c5", action="store_true", help="stages: skip config C5's step (1M x 768 bf16 corpus, beam 30; ~1 min incl. its corpus)")
    ap.add_argument("--sweep", action="store_true",
                    help="stages: also run the two-stage path at 128 / 256 / 1024 / 2048 queries per batch (where the decode chain stops "
                         "being launch-bound); off by default so that the default run stays near 40 s")
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if a.batch is None:
        a.batch = 64 if a.workload == "c3" else 512
    if a.corpus is None:
        a.corpus = 1000000 if a.workload == "c5" else 320000
    if a.beams is None:
        a.beams = 30 if a.workload == "c5" else 10
    if a.workload == "c5":
        a.dtype = "bf16"
    return a


def host_threads():
    """Threads the CPU baseline may really use: scheduler affinity, capped by the cgroup CPU quota."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = max(1, min(n, int(int(quota) / int(period))))
    except Exception:
        pass
    return n


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.lower().startswith("model name"):
                return line.split(":", 1)[1].strip()
    except Exception:
        pass
    return "unknown"


def cpu_baseline(sd, cfg, ids, mask, D, k, budget_s=25.0):
    """The oracle (CPU restatement of the reference path) on a bounded sample of the same workload: the
    sample doubles until one pass costs >= 1/8 of the budget, then is timed (median of 3)."""
    from oracle import t5_ref, retrieval_ref
    torch.set_num_threads(host_threads())
    Dt = torch.from_numpy(D)

    def run(n):
        h = t5_ref.encoder_forward(sd, cfg, torch.from_numpy(ids[:n]), torch.from_numpy(mask[:n]))
        return retrieval_ref.sim_topk(retrieval_ref.cls_pool(h), Dt, k)

    n = 8
    run(n)                                           # warm-up (thread pool, page-in)
    while True:
        t0 = time.perf_counter()
        run(n)
        t = time.perf_counter() - t0
        if t >= budget_s / 8 or n >= ids.shape[0]:
            break
        n = min(n * 2, ids.shape[0])
    ts = [t]
    for _ in range(4):
        t0 = time.perf_counter()
        run(n)
        ts.append(time.perf_counter() - t0)
    med = sorted(ts)[2]
    return {"value": n / med, "unit": "queries/s", "cores": torch.get_num_threads(), "cpu_model": cpu_model(), "kind": "port",
            "sample": f"{n} of the step's queries, whole path (fp32 encoder + Q.D^T top-{k} over all {D.shape[0]} docs), "
                      f"torch-CPU oracle, median of 5 ({med:.2f} s each)"}


def cpu_baseline_two_stage(sd, cfg, ids, mask, D, lookup, R, alphas, n=2, reps=1, budget_s=40.0):
    """The two-stage path on the host cores in the REFERENCE's formulation (generation_utils.py:412-413,520-521 time exactly
    this split; call site main_models.py:1380-1397): oracle generate() with use_cache=False semantics (every position
    recomputed every step) and the full 302-column adaptor head (restricted_head=False), then decode_token -> candidate lookup
    -> the oracle rerank over all alphas.  n queries per call (a bounded sample), `reps` timed calls after none (the first
    call is the measurement when the budget is short: a 100-beam query is ~1.6 TFLOP of head GEMM).
    lookup: cluster string -> list of doc ids (codec.ClusterIndex)."""
    from oracle import beam_ref, codec_ref, retrieval_ref
    torch.set_num_threads(host_threads())
    ids_t, mask_t, Dt = torch.from_numpy(ids[:n]), torch.from_numpy(mask[:n]), torch.from_numpy(np.asarray(D, np.float32))

    def run():
        t0 = time.perf_counter()
        (dec, scores), enc_x = beam_ref.generate(sd, cfg, ids_t, mask_t, R, length_penalty=0.8, restricted_head=False)
        t1 = time.perf_counter()
        names = codec_ref.dec_2d(codec_ref.decode_token(dec.numpy(), cfg.output_vocab_size, cfg.output_vocab_size), R)
        mem = [[m for s_ in row for m in lookup[s_]] for row in names]
        num = [[len(lookup[s_]) for s_ in row] for row in names]
        ran[0] = all(len(m) >= R for m in mem)                 # topk(R) raises on fewer candidates (main_models.py:1625)
        if ran[0]:
            retrieval_ref.rerank(enc_x[::R][:, 0], Dt, mem, num, np.asarray(scores, np.float32).reshape(n, R).tolist(), alphas, R)
        return t1 - t0, time.perf_counter() - t0

    ts, ran = [], [False]
    for _ in range(max(1, reps)):
        ts.append(run())
        if sum(t[1] for t in ts) > budget_s:
            break
    gen_s, tot_s = sorted(ts, key=lambda t: t[1])[len(ts) // 2]
    return {"value": n / tot_s, "unit": "queries/s", "cores": torch.get_num_threads(), "cpu_model": cpu_model(), "kind": "port",
            "generate_s": gen_s, "total_s": tot_s, "rerank_ran": bool(ran[0]),
            "sample": f"{n} quer{'y' if n == 1 else 'ies'} x {R} beams, two-stage path as the reference runs it (use_cache=False, full "
                      f"302-col head, rerank over {len(alphas)} alphas), torch-CPU oracle, median of {len(ts)} ({tot_s:.1f} s each)"}


def recall_at(idx, gold, ks=(1, 10, 100)):
    idx = np.asarray(idx)
    return [float(np.mean([(gold[b] in idx[b, :k]) for b in range(idx.shape[0])])) * 100.0 for k in ks]


def topk_parity(ref_v, ref_i, got_v, got_i, tol=1e-4):
    """SURVEY §8d's top-k rule over every row: values within tol; ids exact wherever neighbouring reference scores
    are more than 2*tol apart; inside a tolerance-tie group the same id set in any order (the last group may be cut by
    k).  Returns (rows with identical id order, permuted slots, rows that break the rule)."""
    ref_v, got_v = np.asarray(ref_v, np.float64), np.asarray(got_v, np.float64)
    ref_i, got_i = np.asarray(ref_i), np.asarray(got_i)
    B, k = ref_v.shape
    identical, permuted, bad = 0, 0, 0
    for r in range(B):
        if not np.allclose(got_v[r], ref_v[r], rtol=tol, atol=tol):
            bad += 1
            continue
        if np.array_equal(ref_i[r], got_i[r]):
            identical += 1
            continue
        j, ok = 0, True
        while j < k and ok:
            e = j
            while e + 1 < k and abs(ref_v[r, e] - ref_v[r, e + 1]) <= 2 * tol * (1 + abs(ref_v[r, e])):
                e += 1
            a, b = ref_i[r, j:e + 1].tolist(), got_i[r, j:e + 1].tolist()
            if e == k - 1:
                permuted += (e - j + 1) - len(set(a) & set(b))
            elif sorted(a) != sorted(b):
                ok = False
            else:
                permuted += sum(1 for x, y in zip(a, b) if x != y)
            j = e + 1
        bad += 0 if ok else 1
    return identical, permuted, bad


def timed(fn, reps=5, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return sorted(ts)[len(ts) // 2]


def stages(dev, cfg, D, D_dev, a):
    """The other stages of the hot path on this GPU (BASELINE configs C3 / C5 and SURVEY §8d's latency-mode point), each
    against the roof that bounds it.  Runs after the headline measurement; nothing here enters `value`."""
    import types
    from gdr_amd import codec, ops, synth
    from gdr_amd.modeling import GDRModel, GDRRetriever
    out = {}
    N, d, k = D.shape[0], cfg.d_model, a.k
    # ---- similarity alone: latency mode is HBM-bound (the corpus is streamed once per call), the batch mode MFMA-bound
    ws = ops.Workspace(dev)
    sim = {}
    for B in (1, 32, 512):
        Qn, _ = synth.make_queries(D[:50000], B, seed=3)
        Q = torch.from_numpy(Qn).to(dev)
        t = timed(lambda: ops.sim_topk(Q, D_dev, k, workspace=ws, exact_on_overflow=False), reps=10, warm=3)
        bytes_ = N * d * 4 + B * d * 4 + B * k * 8
        flops = 2.0 * B * N * d
        e = {"ms": t * 1e3, "queries_per_s": B / t, "algorithmic_mb": bytes_ / 1e6, "gbs": bytes_ / t / 1e9,
             "frac_of_hbm_peak": bytes_ / t / 1e9 / HBM_PEAK_GBS, "tflops": flops / t / 1e12,
             "frac_of_f32_mfma_peak": flops / t / 1e12 / F32_MFMA_PEAK_TFLOPS}
        e["bound"] = "hbm" if bytes_ / (HBM_PEAK_GBS * 1e9) > flops / (F32_MFMA_PEAK_TFLOPS * 1e12) else "mfma"
        sim[f"B{B}"] = e
    out["similarity_topk_f32"] = sim
    # the same calls through the bf16 pre-filter (gdr_sim_topk_prefilter: identical fp32 top-k; the corpus-wide pass streams the bf16
    # image — half the bytes).  frac_of_hbm_peak prices the bytes this form must move (bf16 image + fp32 rescoring rows)
    P = ops.PrefilteredCorpus(D_dev)
    simp = {}
    for B in (1, 32, 512):
        Qn, _ = synth.make_queries(D[:50000], B, seed=3)
        Q = torch.from_numpy(Qn).to(dev)
        t = timed(lambda: ops.sim_topk(Q, P, k, workspace=ws, exact_on_overflow=False), reps=10, warm=3)
        bytes_ = N * d * 2 + B * d * 4 + B * k * 8
        simp[f"B{B}"] = {"ms": t * 1e3, "queries_per_s": B / t, "algorithmic_mb": bytes_ / 1e6, "gbs": bytes_ / t / 1e9,
                         "frac_of_hbm_peak": bytes_ / t / 1e9 / HBM_PEAK_GBS,
                         "speedup_vs_all_fp32": sim[f"B{B}"]["ms"] / (t * 1e3)}
    out["similarity_topk_f32_prefilter"] = simp
    del P
    torch.cuda.empty_cache()
    # ---- docid beam decode (generate()) and the two-stage path, t5-base with the GDR head
    sd = synth.make_state_dict(cfg, seed=1234)
    names, id_depth, offsets, members = synth.make_cluster_ids(N, cluster_size=12, V=30)
    t0 = time.perf_counter()
    model = GDRModel(cfg, sd, dev, ragged=True, prefix_trie=codec.Trie.from_docids(names, 30))
    torch.cuda.synchronize()
    tab = model.prefix_table
    out["prefix_table"] = {"nodes": tab.n_table, "levels": tab.n_levels, "gb": tab.nbytes() / 1e9,
                           "model_load_incl_table_s": time.perf_counter() - t0}
    n_dec = sum(v.numel() for kname, v in sd.items() if kname.startswith("decoder.block") or kname == "decoder.final_layer_norm.weight")
    n_adp = sum(v.numel() for kname, v in sd.items() if kname.startswith("adaptor.layers"))
    V1 = cfg.output_vocab_size + 1
    n_head = V1 * d * d + V1 * d                       # one position's slice of adaptor_linear + lm_head rows
    inner = cfg.num_heads * cfg.d_kv
    mf_dec = cfg.num_decoder_layers * 2 * (6 * d * inner + 2 * d * cfg.d_ff) / 1e6       # MFLOP per row-step: 99.1
    mf_adp = cfg.adaptor_layer_num * 2 * (4 * d * d + 2 * d * cfg.adaptor_ff) / 1e6      # 44.0
    mf_head = 2 * V1 * d * d / 1e6                                                       # 36.6
    args = types.SimpleNamespace(num_return_sequences=10, output_vocab_size=30, max_output_length=10, length_penalty=0.8,
                                 kary=30, position=1, score_rate=[0, 0.5, 1, 1.5, 2, 2.5, 3], loss_func="tanh")
    gen, cpu_two = {}, {}
    ids_np, mask_np = {}, {}
    from gdr_amd import _ffi as _ffi_s
    lib_count = _ffi_s.lib().gdr_launch_count
    # C3 at infer.sh's eval batch, one query x 100 beams, C2's batch; --sweep: the batch sizes that show where the decode chain
    # stops being launch-bound
    sweep = ((64, 10), (1, 100), (512, 10)) + (((128, 10), (256, 10), (1024, 10), (2048, 10)) if a.sweep else ())
    for B, R in sweep:
        ids, mask = synth.make_tokens(B, L=40, seed=11)
        ids_np[(B, R)], mask_np[(B, R)] = ids, mask
        ids, mask = torch.from_numpy(ids).to(dev), torch.from_numpy(mask).to(dev)
        steps = 9
        g = lambda: model.generate(ids, attention_mask=mask, max_length=10, num_beams=R, length_penalty=0.8,   # noqa: E731
                                   num_return_sequences=R, output_scores=True, output_encoder_embedding=True)
        t = timed(g, reps=5, warm=2)
        n0_l = lib_count()
        g()
        torch.cuda.synchronize()
        launches = lib_count() - n0_l                                     # library kernel launches of one generate() call (encoder + decode)
        t_enc = timed(lambda: model.enc.forward(ids, mask, want_pooled=False, ragged=True), reps=5, warm=1)
        rows = B * R
        flops = rows * steps * (mf_dec + mf_adp + mf_head) * 1e6          # the reference-equivalent work (no table)
        # what the timed path EXECUTES: step 0 on one row per query (the R beam rows are identical), the adaptor + head only
        # on the steps the prefix table does not cover (random weights decode 9 digits, the corpus' ids have depth - 1 of
        # them in the table: rows are taken as hits below tab.n_levels and as misses from there on)
        miss_steps = max(0, steps - tab.n_levels)
        flops_exec = ((B + (steps - 1) * rows) * mf_dec + rows * miss_steps * (mf_adp + mf_head)) * 1e6
        wbytes = steps * (n_dec + n_adp + n_head) * 4
        floor = max(flops / (F32_MFMA_PEAK_TFLOPS * 1e12), wbytes / (HBM_PEAK_GBS * 1e9))
        floor_exec = max(flops_exec / (F32_MFMA_PEAK_TFLOPS * 1e12), wbytes / (HBM_PEAK_GBS * 1e9))
        gen[f"B{B}_beam{R}"] = {
            "generate_ms": t * 1e3, "encoder_ms": t_enc * 1e3, "decode_ms": (t - t_enc) * 1e3, "queries_per_s": B / t,
            "kernel_launches_per_call": int(launches),
            "decode_gflop_without_table": flops / 1e9, "decode_weight_gb_streamed": wbytes / 1e9,
            "decode_floor_ms": floor * 1e3, "floor_bound": "mfma" if flops / (F32_MFMA_PEAK_TFLOPS * 1e12) >= wbytes / (HBM_PEAK_GBS * 1e9) else "hbm",
            "frac_of_floor": floor / (t - t_enc), "decode_tflops": flops / (t - t_enc) / 1e12,
            "decode_gflop_executed": flops_exec / 1e9, "decode_floor_executed_ms": floor_exec * 1e3,
            "frac_of_floor_executed": floor_exec / (t - t_enc), "decode_tflops_executed": flops_exec / (t - t_enc) / 1e12,
            "decode_weight_stream_gbs": wbytes / (t - t_enc) / 1e9}
        (dec, _), _ = g()
        a_r = types.SimpleNamespace(**{**vars(args), "num_return_sequences": R})
        strs = sorted({s for s in codec.decode_token(a_r, dec.cpu().numpy())})
        # random weights decode full-length rows that name no cluster: give every decoded string a real 12-doc cluster
        strs = strs[:len(names)]                   # a small --corpus has fewer clusters than a big batch decodes strings
        look = codec.ClusterIndex(strs + names[len(strs):], offsets, members)
        retr = GDRRetriever(model, D_dev, look, a_r)
        batch = {"source_ids": ids, "source_mask": mask}
        t3 = timed(lambda: retr.validation_step_i(batch), reps=5, warm=2)
        c3_par = None
        if B == 64 and not a.no_cpu_baseline and not a.no_parity:   # config C3's step held against the CPU oracle (as --workload c3 does)
            c3_par = two_stage_parity(retr, batch, mask_np[(B, R)], sd, cfg, look, a_r, D_dev, False, None, nq1=2, nq2=64)
        # ---- stage 2 alone (device cluster lookup + in-cluster rerank, SURVEY §8d: bytes/query = Ncand * 768 * 4)
        st = retr._step_launch(batch)
        dci = retr._device_index()
        q_emb = st["enc_h"][:, 0].contiguous()
        bs32 = st["scores"].to(torch.float32).view(B, R)
        _cl, offs2, cids2, stride2 = dci.candidates(st["ids"], B, R)
        ncand = int(offs2[:, R].sum().item())

        def stage2(n=20):
            for _ in range(n):
                _c, o_, i_, s_ = dci.candidates(st["ids"], B, R)
                ops.rerank_topk(q_emb, D_dev, o_, i_, bs32, a_r.score_rate, R, max_cand=s_, cand_stride=s_)

        t2 = timed(stage2, reps=5, warm=1) / 20
        gbytes = ncand * d * 4
        out.setdefault("rerank", {})[f"B{B}_cand{ncand // B}"] = {
            "ms": t2 * 1e3, "queries_per_s": B / t2, "candidates": ncand, "gathered_mb": gbytes / 1e6,
            "gather_gbs": gbytes / t2 / 1e9, "frac_of_hbm_peak": gbytes / t2 / 1e9 / HBM_PEAK_GBS,
            "gather_us_at_hbm_peak": gbytes / (HBM_PEAK_GBS * 1e9) * 1e6}
        nb, depth = (16, 4) if B == 1 else (8, 2) if B <= 64 else (4, 2) if B <= 1024 else (3, 2)   # a stream of batches, `depth` in flight (GDRRetriever.validation_steps)
        tp = timed(lambda: list(retr.validation_steps(iter([batch] * nb), depth=depth)), reps=3, warm=1) / nb
        if B >= 512:           # the grow-only per-stream scratch of a big batch (tens of GB at 2 048 queries) must not pile up
            retr = st = q_emb = bs32 = offs2 = cids2 = None
            model.dec.ws.bufs.clear(), model.enc.ws.bufs.clear(), ops._RERANK_WS.clear()
            torch.cuda.empty_cache()
        skey = "c3_two_stage_infer_sh" if B == 1 else "c3_two_stage" if B == 64 else f"c3_two_stage_B{B}"
        if not a.no_cpu_baseline and B in (1, 64):
            # the CPU path beside this stage (SURVEY §8d "per config"): the oracle in the reference's formulation
            nq = 1 if B == 1 else 2
            cpu_two[skey] = cpu_baseline_two_stage(sd, cfg, ids_np[(B, R)], mask_np[(B, R)], D, look, R, a_r.score_rate, n=nq,
                                                   reps=1 if B == 1 else 3)
        out[skey] = {
            "batch": B, "beams": R, "ms": t3 * 1e3, "queries_per_s": B / t3, "pipelined_depth": depth,
            "pipelined_ms_per_batch": tp * 1e3, "pipelined_queries_per_s": B / tp,
            "generate_ms": t * 1e3, "after_generate_ms": (t3 - t) * 1e3}
        if c3_par is not None:
            out[skey]["parity"] = c3_par
    for skey, cb in cpu_two.items():
        out[skey]["cpu_baseline"] = cb
    out["rerank"]["note"] = ("cluster lookup + dot + per-alpha select (3 launches, 20 calls back to back per timing): launch-bound, not "
                             "bandwidth-bound, at these sizes (compare ms with gather_us_at_hbm_peak)")
    out["c3_two_stage_note"] = ("encoder -> beam decode -> device cluster lookup -> in-cluster rerank over 7 alphas -> host formatting; `ms` = one "
                                "batch start to finish, `pipelined_*` = a stream of batches with `pipelined_depth` in flight on separate HIP "
                                "streams while the host post-processes the previous one")
    best = max((v for kname, v in out.items() if kname.startswith("c3_two_stage") and isinstance(v, dict)), key=lambda v: v["pipelined_queries_per_s"])
    out["c3_best_sustained"] = {"batch": best["batch"], "beams": best["beams"], "queries_per_s": best["pipelined_queries_per_s"],
                                "frac_of_floor_executed": gen[f"B{best['batch']}_beam{best['beams']}"]["frac_of_floor_executed"]}
    out["generate"] = gen
    out["generate"]["mflop_per_row_step"] = {"decoder": mf_dec, "adaptor": mf_adp, "head": mf_head}
    out["generate"]["note"] = ("frac_of_floor prices the REFERENCE-EQUIVALENT work (every row, every step, adaptor + head included) — the "
                               "gain of the exact eliminations shows up in it; frac_of_floor_executed prices only what the kernels "
                               "really run (step-0 de-duplication and table hits subtracted) — the kernel-quality number")
    # ---- the trie-constrained mode (opt-in, generation_utils_previous.py:714-729): every hypothesis is a
    # docid of the corpus, so every beam has ended two steps after the deepest leaf and the call leaves its step loop there
    # (`if all(done): break`, generation_utils.py:836-838) — what a trained model does without the constraint, and what the
    # random weights of the stages above never do (they run all 9 steps)
    from gdr_amd import _ffi
    model.trie = tab.device_trie
    real = codec.ClusterIndex(names, offsets, members)
    con = {}
    for B, R in ((64, 10), (1, 100)):
        ids, mask = synth.make_tokens(B, L=40, seed=11)
        ids, mask = torch.from_numpy(ids).to(dev), torch.from_numpy(mask).to(dev)
        g = lambda: model.generate(ids, attention_mask=mask, max_length=10, num_beams=R, length_penalty=0.8,   # noqa: E731
                                   num_return_sequences=R, output_scores=True, output_encoder_embedding=True)
        n0 = _ffi.lib().gdr_t5_generate_early_exits()
        t = timed(g, reps=5, warm=2)
        t_enc = timed(lambda: model.enc.forward(ids, mask, want_pooled=False, ragged=True), reps=5, warm=1)
        a_r = types.SimpleNamespace(**{**vars(args), "num_return_sequences": R})
        retr_c = GDRRetriever(model, D_dev, real, a_r)
        batch = {"source_ids": ids, "source_mask": mask}
        t3 = timed(lambda: retr_c.validation_step_i(batch), reps=5, warm=2)
        con[f"B{B}_beam{R}"] = {"generate_ms": t * 1e3, "decode_ms": (t - t_enc) * 1e3, "two_stage_ms": t3 * 1e3,
                                "two_stage_queries_per_s": B / t3, "docid_depth": id_depth,
                                "calls_that_left_the_loop_early": int(_ffi.lib().gdr_t5_generate_early_exits() - n0)}
    con["note"] = ("beams constrained to the corpus' docid trie (depth %d + EOS): all queries are done after ~%d of the 9 steps; the "
                   "steps already enqueued skip their linears on the device and the host stops enqueueing" % (id_depth, id_depth + 2))
    out["generate_trie_constrained"] = con
    model.trie = None
    del model, retr
    torch.cuda.empty_cache()
    # ---- bf16 precision mode (config C5): encoder linears + corpus in bf16, fp32 accumulate
    sd_e = {kname: v for kname, v in sd.items() if not kname.startswith(("decoder.", "adaptor", "decode_", "lm_head"))}
    enc16 = ops.T5EncoderHandle(cfg, sd_e, dev, dtype=torch.bfloat16)
    D16 = ops.to_bf16(D_dev)
    ids, mask = synth.make_tokens(a.batch, L=40, seed=11)
    ids, mask = torch.from_numpy(ids).to(dev), torch.from_numpy(mask).to(dev)

    def step16():
        _, pooled = enc16.forward(ids, mask, want_hidden=False, ragged=True, live_rows_hint=int(mask.sum()))
        return ops.sim_topk(pooled, D16, k, workspace=ws, exact_on_overflow=False)

    t = timed(step16, reps=5, warm=2)
    out["bf16_mode_c2_step"] = {"ms": t * 1e3, "queries_per_s": a.batch / t,
                                "note": "ragged encoder with bf16 linear operands + bf16 corpus similarity, fp32 accumulate"}
    del enc16
    torch.cuda.empty_cache()
    # ---- config C5's decode leg: beam 30, bf16 linears in encoder / decoder / adaptor / head (prefix table built in bf16)
    model16 = GDRModel(cfg, sd, dev, prefix_trie=codec.Trie.from_docids(names, 30), dtype=torch.bfloat16)
    ids, mask = synth.make_tokens(64, L=40, seed=11)
    ids, mask = torch.from_numpy(ids).to(dev), torch.from_numpy(mask).to(dev)
    g16 = lambda: model16.generate(ids, attention_mask=mask, max_length=10, num_beams=30, length_penalty=0.8,   # noqa: E731
                                   num_return_sequences=30, output_scores=True)
    t = timed(g16, reps=3, warm=1)
    out["bf16_mode_generate_B64_beam30"] = {"generate_ms": t * 1e3, "queries_per_s": 64 / t,
                                            "note": "C5's decode leg: 1920 beam rows, bf16 linear operands, fp32 accumulate"}
    del model16
    torch.cuda.empty_cache()
    # ---- the passage side of the path: BERT/DPR doc tower, bert-base, 256 passages x 128 tokens, fp32
    from gdr_amd.modeling import EncoderModel
    bc = synth.bert_config(False)
    bsd = synth.make_bert_state_dict(bc)
    tower = EncoderModel.from_state_dict(bc, bsd, dev)
    pids, pmask = synth.make_tokens(256, L=128, vocab_hi=bc["vocab_size"], seed=3, min_len=32)
    live = int(pmask.sum())
    pids, pmask = torch.from_numpy(pids).to(dev), torch.from_numpy(pmask).to(dev)
    t = timed(lambda: tower(passage={"input_ids": pids, "attention_mask": pmask}), reps=5, warm=2)
    Lp, nl, dff, dm = 128, bc["num_layers"], bc["d_ff"], bc["hidden_size"]
    gflop = 256 * (Lp * nl * 2 * (4 * dm * dm + 2 * dm * dff) + nl * 4 * Lp * Lp * dm) / 1e9
    out["doc_tower_bert_base_L128"] = {"ms_per_256_passages": t * 1e3, "passages_per_s": 256 / t, "gflop": gflop,
                                       "tflops": gflop / t / 1e3, "frac_of_f32_mfma_peak": gflop / t / 1e3 / F32_MFMA_PEAK_TFLOPS,
                                       "corpus_320k_embed_s": 320000 / (256 / t),
                                       "note": "padded form (every one of the 128 positions computed); CLS -> pooler; passage lengths "
                                               "uniform 32-128 tokens"}
    # r06: the ragged form (PAD rows not computed, last block on the CLS rows; pooled output bit-identical) and the bf16 precision mode
    # (ragged; bf16 linear operands + bf16-MFMA attention, fp32 accumulate / norms / residual stream) on the same 256 passages
    tower.ragged = True
    tr = timed(lambda: tower.bert.forward(pids, pmask, want_hidden=False, ragged=True, live_rows_hint=live)[1], reps=5, warm=2)
    gflop_live = (live * nl * 2 * (4 * dm * dm + 2 * dm * dff)) / 1e9     # linears over the live rows (the last block's CLS tail not subtracted)
    out["doc_tower_bert_base_L128"]["ragged_f32"] = {
        "ms_per_256_passages": tr * 1e3, "passages_per_s": 256 / tr, "live_token_rows": live, "of_rows": 256 * Lp,
        "linear_gflop_live_rows": gflop_live, "frac_of_f32_mfma_peak_live_linears": gflop_live / tr / 1e3 / F32_MFMA_PEAK_TFLOPS,
        "corpus_320k_embed_s": 320000 / (256 / tr)}
    tower16 = EncoderModel.from_state_dict(bc, bsd, dev, dtype=torch.bfloat16)
    t16 = timed(lambda: tower16.bert.forward(pids, pmask, want_hidden=False, live_rows_hint=live)[1], reps=5, warm=2)
    out["doc_tower_bert_base_L128"]["ragged_bf16"] = {
        "ms_per_256_passages": t16 * 1e3, "passages_per_s": 256 / t16, "live_token_rows": live,
        "frac_of_bf16_mfma_peak_live_linears": gflop_live / t16 / 1e3 / BF16_MFMA_PEAK_TFLOPS,
        "corpus_320k_embed_s": 320000 / (256 / t16),
        "note": "parity: tests/test_gpu_decode.py::test_doc_tower_bf16_mode_vs_oracle_emulation (the build's own bf16 emulation; unpinned)"}
    del tower16
    tower_s = EncoderModel.from_state_dict(bc, bsd, dev, split=True)      # exploratory: fp16 x 2 split linears (fp32-level embeddings)
    ts_ = timed(lambda: tower_s.bert.forward(pids, pmask, want_hidden=False, live_rows_hint=live)[1], reps=5, warm=2)
    p_a = tower.bert.forward(pids, pmask, want_hidden=False, ragged=True)[1]
    p_b = tower_s.bert.forward(pids, pmask, want_hidden=False)[1]
    out["doc_tower_bert_base_L128"]["ragged_split_f16x2"] = {
        "ms_per_256_passages": ts_ * 1e3, "passages_per_s": 256 / ts_, "corpus_320k_embed_s": 320000 / (256 / ts_),
        "pooled_max_abs_diff_vs_fp32": float((p_a - p_b).abs().max()), "pooled_mean_abs": float(p_a.abs().mean()),
        "note": "exploratory: fp32 operands of every linear carried as fp16 hi + fp16 (x - hi) * 2^11 planes (22 bits), fp32 accumulate"}
    del tower_s
    del tower
    torch.cuda.empty_cache()
    # ---- config C5 on this GPU (1M x 768 bf16 corpus, 512 queries, beam 30, bf16 linears): `--workload c5` for 3 steps, with its
    # oracle check (stage 1 on 2 queries against the bf16 emulation, stage 2 on 64), so that the default run's one line carries it
    if not a.no_c5:
        import torch.distributed as dist5
        a5 = argparse.Namespace(**vars(a))
        a5.workload, a5.corpus, a5.batch, a5.beams, a5.dtype, a5.steps, a5.warmup, a5.depth = "c5", 1000000, 512, 30, "bf16", 3, 1, 2
        a5.constrained, a5.parity_queries, a5.full, a5.dump_outputs = False, None, True, None
        a5.parity_only = not (a.no_cpu_baseline or a.no_parity)
        a5.no_parity = a.no_cpu_baseline or a.no_parity
        t5 = time.perf_counter()
        r5, _d5, v5 = two_stage_measure(a5, 0, 1, dev, dist5)
        out["c5_two_stage"] = {"queries_per_s": r5["value"], "ms_per_step": r5["ms_per_step"], "workload": r5["config"]["workload"],
                               "linear_tflops": r5["roofline"]["achieved"], "linear_frac_of_bf16_mfma_peak": r5["roofline"]["frac"],
                               "linear_launches_per_step": r5["roofline"]["launches_per_step"], "kernels": r5["kernels"],
                               "parity": r5["parity"], "parity_violations": v5 if r5["parity"] is not None else None,
                               "stage_wall_s": time.perf_counter() - t5, "corpus_setup_s": r5["config"]["corpus_setup_s"]}
    return out


def two_stage_parity(retr, batch, mask_np, sd, cfg, look, args, D_dev, bf16, tree, nq1, nq2):
    """The oracle check of a --workload c3 / c5 line (N = 1): the step the line times, held against the CPU oracle on a bounded
    sample of its queries, with the rules the -m gpu tests use (oracle/parity_rules.py).
      stage 1 (first nq1 queries): beam hypotheses as token rows.  fp32: oracle generate() on the same tokens — ranks exact
        outside 1e-4 tolerance ties, scores within 1e-4.  bf16 (C5): the oracle's emulation of the decode path's rounding points
        (t5_ref.bf16_linears) on the GPU's own encoder states; the score gap on shared hypotheses is MEASURED (<= 5e-3) and is the
        absolute tie tolerance of hypothesis_lists_match; an id outside the emulation's list must be explained by a tie at a
        cut of the emulation's own search.
      stage 2 (first nq2 queries): oracle rerank on the candidate rows as the GPU holds them (bf16 rows widened exactly) and the
        GPU's stage-1 order and scores: values within 1e-4, ids exact outside 1e-4 ties, for every alpha.
    Returns the `parity` object; violations are counted, the caller exits non-zero on any."""
    from oracle import beam_ref, codec_ref, retrieval_ref, t5_ref, parity_rules as pr
    from gdr_amd import ops
    R, V, TOL = args.num_return_sequences, args.output_vocab_size, 1e-4
    state = retr._step_launch(batch)
    out = retr._step_finish(state)
    B = batch["source_ids"].shape[0]
    nq1, nq2 = min(nq1, B), min(nq2, B)
    got_scores = np.array(out["inf_result_batch_prob"], np.float64).reshape(B, R)
    outs, _ = ops.finish_generate_output(state["ids"], state["lens"], state["scores"], args.max_output_length)
    outs = outs.cpu().numpy().reshape(B, R, -1)

    def canon(row):                     # START, tokens, [EOS, PAD...] -> the hypothesis without its padding
        row = [int(t) for t in row]
        return tuple(row[:2 + row[1:].index(1)]) if 1 in row[1:] else tuple(row)

    got_rows = [[canon(r) for r in outs[q]] for q in range(nq1)]
    ids_t, mask_t = batch["source_ids"][:nq1].cpu(), torch.from_numpy(mask_np[:nq1])
    trace, ptrace = [], []
    if bf16:
        idx = torch.arange(nq1).view(-1, 1).repeat(1, R).view(-1)
        enc_x, mask_x = state["enc_h"][:nq1].float().cpu().index_select(0, idx), mask_t.index_select(0, idx)

        def step(seq):
            with t5_ref.bf16_linears():
                return t5_ref.decode_logits(sd, cfg, seq, enc_x, mask_x, restricted=True)

        rd, rs = beam_ref.beam_search(step, nq1, R, cfg.decode_vocab_size, args.max_output_length, args.length_penalty, R,
                                      decode_tree=tree, trace=trace, prefix_trace=ptrace)
    else:
        (rd, rs), _ = beam_ref.generate(sd, cfg, ids_t, mask_t, R, max_length=args.max_output_length,
                                        length_penalty=args.length_penalty, restricted_head=True, decode_tree=tree)
    ref_rows = [[canon(r) for r in rd.numpy().reshape(nq1, R, -1)[q]] for q in range(nq1)]
    rs2 = np.array(rs, np.float64).reshape(nq1, R)
    gap, shared, moved, foreign, bad1 = 0.0, 0, 0, 0, 0
    for q in range(nq1):
        where = {x: i for i, x in enumerate(ref_rows[q])}
        hits = [abs(got_scores[q, p] - rs2[q, where[x]]) for p, x in enumerate(got_rows[q]) if x in where]
        gap, shared = max([gap] + hits), shared + len(hits)
    tie = max(gap, 2e-4) if bf16 else TOL
    for q in range(nq1):
        try:
            if bf16:
                assert gap <= 5e-3, f"score gap {gap:.2e} on shared hypotheses"
                m, f, _sz = pr.hypothesis_lists_match(
                    ref_rows[q], rs2[q], got_rows[q], tie,
                    explain_foreign=lambda row, q=q: pr.beam_cut_explains_absence(trace, ptrace, q, R, cfg.decode_vocab_size, list(row), tie,
                                                                                  lp=args.length_penalty, final_cut=rs2[q, -1]))
                moved, foreign = moved + m, foreign + f
            else:
                moved += pr.ranked_lists_match(ref_rows[q], rs2[q], got_rows[q], TOL)
                np.testing.assert_allclose(got_scores[q], rs2[q], rtol=TOL, atol=TOL)
        except AssertionError as e:
            bad1 += 1
            print(f"bench parity: stage 1, query {q}: {str(e)[:300]}", file=sys.stderr)
    if bf16 and shared < 0.95 * nq1 * R:
        bad1 += 1
    # ---- stage 2: the oracle rerank on the rows the GPU gathered, in the GPU's stage-1 order
    q_emb = state["enc_h"][:nq2, 0].float().cpu()
    cand = [[int(m) for s_ in out["clusters"][b] for m in look[s_]] for b in range(nq2)]
    num = [[len(look[s_]) for s_ in out["clusters"][b]] for b in range(nq2)]
    flat = torch.tensor(sorted({m for c in cand for m in c}), dtype=torch.long)
    rows = D_dev[flat.to(D_dev.device)].float().cpu()
    remap = {int(m): j for j, m in enumerate(flat.tolist())}
    bad2, permuted = 0, 0
    for b in range(nq2):
        if len(cand[b]) < R:
            continue                                            # topk(R) raises in the reference on fewer candidates
        ref = retrieval_ref.rerank(q_emb[b:b + 1], rows, [[remap[m] for m in cand[b]]], [num[b]],
                                   [got_scores[b].astype(np.float32).tolist()], args.score_rate, R)[0]
        try:
            for ai in range(len(args.score_rate)):
                ref_ids = [str(int(flat[j])) for j in ref[ai][1].tolist()]
                permuted += pr.ranked_lists_match(ref_ids, ref[ai][0].numpy(), out["doc_ids"][b][ai], TOL)
                np.testing.assert_allclose(out["rerank_values"][b, ai].cpu().numpy(), ref[ai][0].numpy(), rtol=TOL, atol=TOL)
        except AssertionError as e:
            bad2 += 1
            print(f"bench parity: stage 2, query {b}: {str(e)[:300]}", file=sys.stderr)
    return {"stage1_queries": nq1, "stage1_ids_shared": shared, "stage1_ids_total": nq1 * R, "stage1_moved_inside_ties": moved,
            "stage1_foreign_explained_by_a_cut_tie": foreign, "stage1_rows_violating": bad1, "score_gap": gap,
            "stage2_queries": nq2, "stage2_permuted_slots_inside_ties": permuted, "stage2_rows_violating": bad2,
            "against": ("oracle bf16 emulation on the GPU's encoder states; tie tolerance = the measured gap" if bf16 else
                        "oracle generate() + rerank, fp32, tol 1e-4")}


def stages_summary(st):
    """A dozen-odd scalars of the stages for the headline line (the full object goes to the #stages line)."""
    g, sim = st["generate"], st["similarity_topk_f32"]
    return {"c3_B64_beam10_qps": st["c3_two_stage"]["queries_per_s"],
            "c3_best_sustained_qps": st["c3_best_sustained"]["queries_per_s"],
            "B64_beam10_decode_ms": g["B64_beam10"]["decode_ms"],
            "B64_beam10_frac_of_floor_executed": g["B64_beam10"]["frac_of_floor_executed"],
            "B1_beam100_decode_ms": g["B1_beam100"]["decode_ms"],
            "B64_beam10_launches": g["B64_beam10"]["kernel_launches_per_call"],
            "bf16_c2_qps": st["bf16_mode_c2_step"]["queries_per_s"],
            "bf16_B64_beam30_generate_ms": st["bf16_mode_generate_B64_beam30"]["generate_ms"],
            "sim_B1_ms": sim["B1"]["ms"], "sim_B32_ms": sim["B32"]["ms"],
            "sim_B32_frac_of_hbm_peak": sim["B32"]["frac_of_hbm_peak"],
            "sim_B1_prefilter_ms": st["similarity_topk_f32_prefilter"]["B1"]["ms"],
            "sim_B32_prefilter_ms": st["similarity_topk_f32_prefilter"]["B32"]["ms"],
            "doc_tower_frac_of_f32_mfma_peak": st["doc_tower_bert_base_L128"]["frac_of_f32_mfma_peak"],
            "doc_tower_320k_embed_s": [st["doc_tower_bert_base_L128"][k_]["corpus_320k_embed_s"] if k_ else
                                       st["doc_tower_bert_base_L128"]["corpus_320k_embed_s"] for k_ in ("", "ragged_f32", "ragged_bf16")],
            "doc_tower_split_f16x2_embed_s": st["doc_tower_bert_base_L128"]["ragged_split_f16x2"]["corpus_320k_embed_s"],
            "B1_beam100_launches": g["B1_beam100"]["kernel_launches_per_call"],
            "B1_beam100_frac_of_floor_executed": g["B1_beam100"]["frac_of_floor_executed"],
            "c3_parity_violations": (lambda p_: None if p_ is None else p_["stage1_rows_violating"] + p_["stage2_rows_violating"])(
                st["c3_two_stage"].get("parity")),
            "c5_qps": (st.get("c5_two_stage") or {}).get("queries_per_s"),
            "c5_linear_frac": (st.get("c5_two_stage") or {}).get("linear_frac_of_bf16_mfma_peak"),
            "c5_parity_violations": (st.get("c5_two_stage") or {}).get("parity_violations")}


def fence(dist):
    torch.cuda.synchronize()
    if dist.is_initialized():
        dist.barrier()
    torch.cuda.synchronize()


def launch_self(a):
    """`python bench.py --gpus N` with no RANK in the environment: this process (no GPU call made) starts the N ranks as fresh
    children under torch.distributed.run, lets rank 0's JSON line through to stdout (everything else the ranks print goes to
    stderr) and exits with the launcher's code."""
    from gdr_amd import launch
    tail = [x for x in sys.argv[1:] if x != "--launcher"]

    def relay(line):
        dst = sys.stdout if line.startswith(("{", "#stages ")) else sys.stderr
        dst.write(line)
        dst.flush()

    rc, _ = launch.spawn_ranks(a.gpus, tail, script=os.path.abspath(__file__), relay=relay)
    raise SystemExit(rc)


def init_ranks(a):
    """(rank, world, device, dist) of this process; under torch.distributed.run the RCCL group is set up (and warmed: RCCL
    connects lazily) before anything is timed."""
    import torch.distributed as dist
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != a.gpus:
        a.gpus = world
    n_dev = torch.cuda.device_count()                                    # counting devices does not initialise the GPU
    if a.backend == "nccl" and world > max(1, n_dev):
        # RCCL refuses two ranks on one device; folding ranks onto the GPUs that exist would print a number that is not a scaling
        # measurement under the product backend's name
        raise SystemExit(f"bench: --backend nccl with WORLD_SIZE {world} needs {world} GPUs, this node has {n_dev} "
                         "(use --backend gloo to let ranks share a GPU: a functional run, not a scaling measurement)")
    local_rank %= max(1, n_dev)                                          # more ranks than GPUs (--backend gloo): they share
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    launched = "RANK" in os.environ and "MASTER_PORT" in os.environ      # under torch.distributed.run
    if world > 1 or launched:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if a.backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(a.backend)
        _t = torch.ones(1, device=dev)
        dist.all_reduce(_t)                  # communicator set-up stays out of the timed region even with --warmup 0
        torch.cuda.synchronize()
    torch.set_grad_enabled(False)
    return rank, world, dev, dist


def two_stage_main(a):
    """--workload c3 / c5: the two-stage GDR path (main_models.py:1337-1642) per GPU, stage 2 over the row-sharded corpus."""
    rank, world, dev, dist = init_ranks(a)
    result, detail, violations = two_stage_measure(a, rank, world, dev, dist)
    if rank == 0:
        emit(result, detail if a.full else None)
        if violations:
            raise SystemExit(f"bench: {violations} queries of the step differ from the CPU oracle outside the parity rule")
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


def two_stage_measure(a, rank, world, dev, dist):
    """One --workload c3 / c5 measurement on this rank: (result, detail, parity violations) on rank 0, (None, None, 0) elsewhere.
    Also called by stages() of the default run for C5's numbers (1 GPU, a few steps), so that the driver's one line carries them."""
    import types
    from gdr_amd import codec, ops, synth, _ffi
    from gdr_amd.config import GDRConfig
    from gdr_amd.dist import ShardedIndex, shard_bounds
    from gdr_amd.modeling import GDRModel, GDRRetriever

    cfg = GDRConfig.base()
    bf16 = a.dtype == "bf16"
    R, B = a.beams, a.batch
    sd = synth.make_state_dict(cfg, seed=1234)
    names, id_depth, offsets, members = synth.make_cluster_ids(a.corpus, cluster_size=12, V=30)
    trie = codec.Trie.from_docids(names, 30)
    model = GDRModel(cfg, sd, dev, ragged=True, prefix_trie=trie, trie=trie if a.constrained else None,
                     dtype=torch.bfloat16 if bf16 else torch.float32)
    lo, hi = shard_bounds(a.corpus, world, rank, cluster_size=12)
    t_c = time.perf_counter()
    D = synth.make_corpus(a.corpus, cfg.d_model, rows=(lo, hi) if world > 1 else None)   # N > 1: this rank's rows only (bit-identical
    t_corpus = time.perf_counter() - t_c                                                 # to the slice of the whole corpus)
    D_dev = torch.from_numpy(D).to(dev)
    if bf16:
        D_dev = ops.to_bf16(D_dev)
    ids_all, mask_all = synth.make_tokens(B * world, L=40, seed=11)
    ids = torch.from_numpy(ids_all[rank * B:(rank + 1) * B]).to(dev)
    mask = torch.from_numpy(mask_all[rank * B:(rank + 1) * B]).to(dev)
    args = types.SimpleNamespace(num_return_sequences=R, output_vocab_size=30, max_output_length=10, length_penalty=0.8,
                                 kary=30, position=1, score_rate=[0, 0.5, 1, 1.5, 2, 2.5, 3], loss_func="tanh")
    if a.constrained:
        look = codec.ClusterIndex(names, offsets, members)
    else:
        # random weights decode full-length rows that name no cluster: every string this rank's batch decodes gets a real
        # 12-doc cluster, so stage 2 sees C3's candidate counts (R x 12 per query).  The index may differ per rank — the
        # exchange carries doc ids, only the block width (R x largest cluster) must agree
        (dec, _), _ = model.generate(ids, attention_mask=mask, max_length=10, num_beams=R, length_penalty=0.8,
                                     num_return_sequences=R, output_scores=True)
        strs = sorted(set(codec.decode_token(args, dec.cpu().numpy())))[:len(names)]
        look = codec.ClusterIndex(strs + names[len(strs):], offsets, members)
    sharded = ShardedIndex(D_dev, lo) if (world > 1 or dist.is_initialized()) else None
    retr = GDRRetriever(model, None if sharded is not None else D_dev, look, args, sharded=sharded)
    batch = {"source_ids": ids, "source_mask": mask}

    def run(n):
        outs = list(retr.validation_steps(iter([batch] * n), depth=max(1, a.depth)))
        return outs[-1] if outs else None

    run(max(1, a.depth))           # set-up, not warm-up: every stream of the pipeline allocates its scratch (GBs of hipMalloc) once
    if a.warmup:
        run(a.warmup)
    fence(dist)
    t0 = time.perf_counter()
    last = run(a.steps)
    fence(dist)
    dt = time.perf_counter() - t0
    if dist.is_initialized():
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    if a.dump_outputs and rank == 0 and last is not None:      # this rank's queries: per-alpha rerank lists and beam scores
        dump_outputs(a.dump_outputs, {"rerank_values": last["rerank_values"], "rerank_doc_ids": last["doc_id_tensor"],
                                      "beam_scores": np.asarray(last["inf_result_batch_prob"], np.float64).reshape(B, R)})
    n_cand = int(sum(len(look[s_]) for s_ in last["clusters"][0])) if last is not None else 0
    # --full: the dominant kernel class (every linear: encoder, decoder, adaptor, head) from a PROFILED replay of the same steps
    # right after the timed region — ~1 100 launches per step, each bracketed by two hipEvents, would slow a launch-bound chain
    # if they were recorded inside it
    if a.full:
        lib = _ffi.lib()
        n_prof = min(a.steps, 3)
        _ffi.check(lib.gdr_prof_enable(4000 * n_prof * max(1, a.depth)), "gdr_prof_enable")
        run(n_prof)
        torch.cuda.synchronize()
        n_l, ms_l, w_l = (C.c_int64 * 8)(), (C.c_double * 8)(), (C.c_double * 8)()
        lost = lib.gdr_prof_collect(n_l, ms_l, w_l)
        if lost < 0:
            _ffi.check(lost, "gdr_prof_collect")
    if rank == 0:
        peak = BF16_MFMA_PEAK_TFLOPS if bf16 else F32_MFMA_PEAK_TFLOPS
        tag = a.workload.upper() + ("/constrained" if a.constrained else "") + ("/sharded" if sharded is not None else "")
        result = {
            "metric": "queries/sec on NQ-320k (768-d)" if a.workload == "c3" else "queries/sec on a 1Mx768 corpus (TriviaQA-scale)",
            "value": B * world * a.steps / dt, "unit": "queries/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": dt / a.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": a.dtype, "data": "synthetic",
            "config": {"workload": f"{tag}: two-stage GDR, {B} q/GPU, beam {R}, {a.corpus}x{cfg.d_model} {'bf16' if bf16 else 'fp32'} corpus",
                       "dist_backend": a.backend if dist.is_initialized() else None,
                       "batch_per_gpu": B, "global_batch": B * world, "beams": R, "seq_len": 40, "corpus_rows": a.corpus,
                       "dim": cfg.d_model, "k": R, "alphas": 7, "candidates_per_query": n_cand, "pipeline_depth": max(1, a.depth),
                       "docid_depth": id_depth, "corpus_setup_s": round(t_corpus, 2), "corpus_rows_on_host": int(D.shape[0])},
            "roofline": None, "kernels": None, "cpu_baseline": None, "parity": None, "recall": None,
        }
        if a.full:
            lin_tf = w_l[0] / (ms_l[0] * 1e-3) / 1e12 if ms_l[0] > 0 else 0.0
            result["roofline"] = {
                "bound": "mfma",
                "kernel": ("every linear of the step (encoder, decoder, adaptor, head): gdr::gemm_nt_bf16_*" if bf16 else
                           "every linear of the step: gdr::gemm_nt_f32_small_kernel (decode rows) + persistent / stream-K (encoder)"),
                "achieved": lin_tf, "peak": peak, "unit": "TFLOP/s", "frac": lin_tf / peak, "traffic": None,
                "launches_per_step": int(n_l[0]) / n_prof, "avg_launch_ms": ms_l[0] / max(1, int(n_l[0])),
                "linear_ms_per_step": ms_l[0] / n_prof, "events_lost": int(lost)}
            result["kernels"] = {"attention_ms_per_step": ms_l[3] / n_prof, "rerank_dot_ms_per_step": ms_l[6] / n_prof,
                                 "rerank_select_ms_per_step": ms_l[5] / n_prof, "splitk_reduce_ms_per_step": ms_l[7] / n_prof}
        detail = {"config_note": "a step = one batch per GPU through validation_step_i: ragged t5-base encoder -> docid beam decode "
                  f"(beam {R}, 9 steps, prefix table) -> device cluster lookup -> in-cluster rerank over 7 alphas "
                  f"(top-{R}) -> host formatting; {max(1, a.depth)} batches in flight; corpus resident in HBM"
                  + ("; beams constrained to the corpus' docid trie" if a.constrained else
                     "; unconstrained beams of random weights run all 9 steps, every decoded string is mapped to a real 12-doc cluster")
                  + (f"; corpus row-sharded {world} ways, stage 2 = one all-gather of queries + candidate blocks, per-shard "
                     "scoring, one all-to-all of the packed lists, merge" if sharded is not None else ""),
                  "roofline_source": f"profiled replay of {n_prof} step(s) after the timed region (hipEvent pairs on the launch streams; "
                                     "summed durations of two overlapping chains can exceed the step's wall time)"} if a.full else None
        violations = 0
        parity_only = getattr(a, "parity_only", False)        # stages(): the oracle check without the CPU timing leg
        if a.full and world == 1 and not a.no_parity and (parity_only or not a.no_cpu_baseline):
            tree = None
            if a.constrained:
                from oracle import beam_ref, codec_ref
                tree = beam_ref.build_trie([codec_ref.encode_single_newid(s_, kary=30) for s_ in names])
            result["parity"] = two_stage_parity(retr, batch, mask_all, sd, cfg, look, args, D_dev, bf16, tree,
                                                nq1=a.parity_queries[0] if a.parity_queries else (2 if R > 10 else 4),
                                                nq2=a.parity_queries[1] if a.parity_queries else 64)
            violations = result["parity"]["stage1_rows_violating"] + result["parity"]["stage2_rows_violating"]
        if a.full and world == 1 and not a.no_cpu_baseline and not parity_only and not violations:
            result["cpu_baseline"] = cpu_baseline_two_stage(sd, cfg, ids_all, mask_all, D, look, R, args.score_rate,
                                                            n=1 if R > 10 else 2, reps=1 if R > 10 else 3)
        return result, detail, violations
    return None, None, 0


def main():
    a = parse()
    if (a.gpus > 1 or a.launcher) and "RANK" not in os.environ:
        launch_self(a)
    if a.workload != "c2":
        return two_stage_main(a)
    rank, world, dev, dist = init_ranks(a)

    from gdr_amd import ops, synth, _ffi
    from gdr_amd.config import GDRConfig
    from gdr_amd.dist import ShardedIndex, shard_bounds
    cfg = GDRConfig.base()
    sd = synth.make_state_dict(cfg, seed=1234, with_decoder=False)
    bf16 = a.dtype == "bf16"
    form_terms = {"f32": 0, "f16x2": 2, "bf16x3": 6, "bf16x3-16": 3}[a.encoder_form]
    if form_terms and (bf16 or a.encoder != "ragged"):
        raise SystemExit("bench: --encoder-form is a form of the fp32 ragged encoder (--dtype f32, --encoder ragged)")
    enc = ops.T5EncoderHandle(cfg, sd, dev, dtype=torch.bfloat16 if bf16 else torch.float32, split=form_terms)
    lo, hi = shard_bounds(a.corpus, world, rank, cluster_size=12)
    t_c = time.perf_counter()
    D = synth.make_corpus(a.corpus, cfg.d_model, rows=(lo, hi) if world > 1 else None)   # N > 1: this rank's rows only (bit-identical
    t_corpus = time.perf_counter() - t_c                                                 # to the slice of the whole corpus)
    D_dev = torch.from_numpy(D).to(dev)
    if bf16:
        D_dev = ops.to_bf16(D_dev)
    D_raw = D_dev                                    # the corpus tensor itself (stages, the other similarity form)
    use_pre = a.sim_prefilter == "bf16" and not bf16
    if use_pre:
        D_dev = ops.PrefilteredCorpus(D_raw)
    index = ShardedIndex(D_dev, lo, exact=False)     # no host sync in the timed region; the status is checked after it
    ids_all, mask_all = synth.make_tokens(a.batch * world, L=40, seed=11)
    ids = torch.from_numpy(ids_all[rank * a.batch:(rank + 1) * a.batch]).to(dev)
    mask = torch.from_numpy(mask_all[rank * a.batch:(rank + 1) * a.batch]).to(dev)
    ragged = a.encoder == "ragged"
    live_rows = int(mask_all[rank * a.batch:(rank + 1) * a.batch].sum())      # token rows that are not PAD (host-side metadata)

    pending = [None]

    def step():
        """One batch through the path.  N > 1: the exchange + merge of this batch is left in flight on a side stream and
        joined at the start of the next step's search, i.e. it overlaps the next batch's encoder."""
        _, pooled = enc.forward(ids, mask, want_hidden=False, ragged=ragged, live_rows_hint=live_rows)
        q_all = index.gather_queries(pooled)
        if a.replicated_merge:
            return index.search(q_all, a.k, return_status=True)
        prev = pending[0].wait() if pending[0] is not None else None
        pending[0] = index.search_own_async(q_all, a.k)
        return prev

    def drain():
        out = pending[0].wait() if pending[0] is not None else None
        pending[0] = None
        return out

    for _ in range(a.warmup):
        step()
    drain()
    lib = _ffi.lib()
    launches_per_step = 13 * cfg.num_layers + 16        # per layer: 4 linears x (main + tail + reduce) + attention
    _ffi.check(lib.gdr_prof_enable(launches_per_step * a.steps + 16), "gdr_prof_enable")
    fence(dist)
    t0 = time.perf_counter()
    out = None
    pe = max(1, a.prof_every)
    for i in range(a.steps):
        lib.gdr_prof_gate(1 if i % pe == 0 else 0)       # a systematic sample of the steps carries the event pairs
        r = step()
        out = r if r is not None else out
    lib.gdr_prof_gate(1)
    r = drain()                                          # the last batch's exchange completes inside the timed region
    out = r if r is not None else out
    fence(dist)
    dt = time.perf_counter() - t0
    n_l, ms_l, w_l = (C.c_int64 * 8)(), (C.c_double * 8)(), (C.c_double * 8)()
    _ffi.check(lib.gdr_prof_collect(n_l, ms_l, w_l), "gdr_prof_collect")
    if dist.is_initialized():
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    overflowed = int(out[2].sum().item())     # gdr_sim_topk status: rows whose candidate list overflowed (subset top-k)
    if overflowed:
        raise SystemExit(f"bench: {overflowed} queries overflowed their candidate lists — the step did not compute "
                         "the exact top-k (use exact_on_overflow=True for such data)")
    if a.dump_outputs and rank == 0:                     # this rank's queries: top-k values and global doc ids
        dump_outputs(a.dump_outputs, {"topk_values": out[0], "topk_ids": out[1]})
    # ---- the same step with the OTHER similarity form — all-fp32 when the headline runs the bf16 pre-filter (the default), the
    # pre-filter when it runs all-fp32 (--sim-prefilter off) — timed AFTER the headline region with the same protocol, reported
    # beside it, never as `value`.  Both forms return the top-k of the fp32 scores for every input (tests/test_gpu_prefilter.py).
    pre = None
    if a.full and world == 1 and not bf16 and not a.no_stages:
        P = D_dev if use_pre else ops.PrefilteredCorpus(D_raw)
        index_p = ShardedIndex(D_raw if use_pre else P, lo, exact=False)

        def step_p():
            _, pooled = enc.forward(ids, mask, want_hidden=False, ragged=ragged, live_rows_hint=live_rows)
            return index_p.search(pooled, a.k, return_status=True)

        for _ in range(max(1, a.warmup)):
            step_p()
        fence(dist)
        t0p = time.perf_counter()
        for _ in range(a.steps):
            outp = step_p()
        fence(dist)
        dtp = time.perf_counter() - t0p
        pre = {"form": "all_fp32" if use_pre else "bf16_prefilter", "queries_per_s": a.batch * a.steps / dtp,
               "ms_per_step": dtp / a.steps * 1e3, "flagged_rows": int(outp[2].sum().item()), "extra_hbm_mb": P.D16.numel() * 2 / 1e6}

    # ---- the same step with the PADDED encoder (every one of the batch x 40 token rows through all 48 linears, as the reference
    # computes it): the reference-equivalent-work number beside the headline's exact work elimination; same protocol, own roofline
    padded = None
    if a.full and world == 1 and not bf16 and ragged and not a.no_stages and not form_terms:
        def step_pad():
            _, pooled = enc.forward(ids, mask, want_hidden=False, ragged=False)
            return index.search(pooled, a.k, return_status=True)

        for _ in range(max(1, a.warmup)):
            step_pad()
        _ffi.check(lib.gdr_prof_enable(launches_per_step * a.steps + 16), "gdr_prof_enable")
        fence(dist)
        t0q = time.perf_counter()
        for i in range(a.steps):
            lib.gdr_prof_gate(1 if i % pe == 0 else 0)
            step_pad()
        lib.gdr_prof_gate(1)
        fence(dist)
        dtq = time.perf_counter() - t0q
        n_q, ms_q, w_q = (C.c_int64 * 8)(), (C.c_double * 8)(), (C.c_double * 8)()
        _ffi.check(lib.gdr_prof_collect(n_q, ms_q, w_q), "gdr_prof_collect")
        lin_tf = w_q[0] / (ms_q[0] * 1e-3) / 1e12 if ms_q[0] > 0 else 0.0
        padded = {"queries_per_s": a.batch * a.steps / dtq, "ms_per_step": dtq / a.steps * 1e3, "token_rows": a.batch * 40,
                  "linear_tflops": lin_tf, "linear_frac_of_f32_mfma_peak": lin_tf / F32_MFMA_PEAK_TFLOPS,
                  "linear_launches_timed": int(n_q[0])}

    # ---- EXPLORATORY, beside the headline and never instead of it: the same step with every encoder linear in the
    # split-bf16 form (gdr_t5_encoder_forward_ragged_split: fp32 operands carried as three bf16 planes, six bf16 MFMA products, fp32
    # accumulate — the fp32 linear's error against float64, not its bits).  Its top-k lists are held to the fp32 step's by the top-k rule.
    split = None
    if a.full and world == 1 and not bf16 and ragged and not a.no_stages and not form_terms:
        _, p_f = enc.forward(ids, mask, want_hidden=False, ragged=True, live_rows_hint=live_rows)
        out_f = index.search(p_f, a.k, return_status=True)
        split = {}
        # 2: fp16 x 2 planes, 22 bits carried, three blocks (hi.hi + 2^-11 (hi.lo' + lo'.hi)): error against float64 BELOW the fp32 MFMA
        # linear's own; 6: bf16 x 3, 24 bits, six blocks; 3: the first three bf16 blocks, 16 bits — NARROWER than fp32
        for terms in (6, 2, 3):
            enc_s = ops.T5EncoderHandle(cfg, sd, dev, split=terms)

            def step_s():
                _, pooled = enc_s.forward(ids, mask, want_hidden=False, ragged=True, live_rows_hint=live_rows)
                return pooled, index.search(pooled, a.k, return_status=True)

            for _ in range(max(1, a.warmup) + 3):      # a new handle: its first calls allocate scratch and load three kernel variants
                step_s()
            _ffi.check(lib.gdr_prof_enable(launches_per_step * a.steps + 16), "gdr_prof_enable")
            fence(dist)
            t0s = time.perf_counter()
            for i in range(a.steps):
                lib.gdr_prof_gate(1 if i % pe == 0 else 0)
                p_s, out_s = step_s()
            lib.gdr_prof_gate(1)
            fence(dist)
            dts = time.perf_counter() - t0s
            n_s, ms_s, w_s = (C.c_int64 * 8)(), (C.c_double * 8)(), (C.c_double * 8)()
            _ffi.check(lib.gdr_prof_collect(n_s, ms_s, w_s), "gdr_prof_collect")
            ident, perm, bad_s = topk_parity(out_f[0].cpu().numpy(), out_f[1].cpu().numpy(), out_s[0].cpu().numpy(), out_s[1].cpu().numpy())
            lin_eq = w_s[0] / (ms_s[0] * 1e-3) / 1e12 if ms_s[0] > 0 else 0.0      # fp32-equivalent flops (2 M N K) per second
            split["f16x2" if terms == 2 else f"terms{terms}"] = {
                "queries_per_s": a.batch * a.steps / dts, "ms_per_step": dts / a.steps * 1e3, "significand_bits_carried": {2: 22, 6: 24, 3: 16}[terms],
                "linear_fp32_equiv_tflops": lin_eq, "linear_16bit_mfma_tflops": (3 if terms == 2 else terms) * lin_eq,
                "linear_frac_of_16bit_mfma_peak": (3 if terms == 2 else terms) * lin_eq / BF16_MFMA_PEAK_TFLOPS,
                "pooled_max_abs_diff_vs_fp32": float((p_s - p_f).abs().max()), "pooled_mean_abs": float(p_f.abs().mean()),
                "topk_vs_fp32_step": {"rows": a.batch, "ids_identical_rows": ident, "permuted_slots_inside_1e-4_ties": perm,
                                      "rows_violating_tie_rule": bad_s}}
            del enc_s
            torch.cuda.empty_cache()
        split["note"] = ("EXPLORATORY, never the headline: encoder linears with fp32 operands as 16-bit planes on the bf16 / fp16 MFMA path, fp32 "
                         "accumulate; f16x2 = fp16 hi + fp16 (x - hi) * 2^11 (22 bits; hi.hi + 2^-11 (hi.lo' + lo'.hi): against float64 the error is "
                         "BELOW the fp32 MFMA linear's own, tools/exp_split_bf16.py); terms6 = bf16 hi.hi + hi.mid + mid.hi + hi.lo + lo.hi + mid.mid "
                         "(24 bits); terms3 = the first three (16 bits: narrower than fp32, inside the path's 2e-4 / 1e-4 parity tolerances here); "
                         "norms / attention / residual stream / similarity are the headline's; tests: test_encoder_split_bf16_form_…")

    total_q = a.batch * world * a.steps
    ms_per_step = dt / a.steps * 1e3
    n_prof_steps = len(range(0, a.steps, max(1, a.prof_every)))
    if rank == 0:
        def cls(c):
            if n_l[c] == 0:
                return None
            avg_ms = ms_l[c] / n_l[c]
            avg_work = w_l[c] / n_l[c]
            return {"launches": int(n_l[c]), "avg_ms": avg_ms, "gflop_per_launch": avg_work / 1e9,
                    "tflops": avg_work / (avg_ms * 1e-3) / 1e12, "share_of_step": ms_l[c] / n_prof_steps / (dt / a.steps * 1e3)}

        lin, smp, flt, att, red = cls(0), cls(1), cls(2), cls(3), cls(7)
        # roofline.traffic comes from a committed PMC collection (profiles/traffic.json, tools/summarize_profiles.py), not from this
        # run: it carries the hash of the GEMM source it was counted on, and the line says so when that is no longer the source here
        traffic, traffic_stale = None, None
        tpath = os.path.join(REPO, "profiles", "traffic.json")
        if os.path.exists(tpath):
            try:
                import hashlib
                tj = json.load(open(tpath))
                traffic = tj.get("linear_gemm_bytes_per_launch_ragged" if ragged else "linear_gemm_bytes_per_launch")
                with open(os.path.join(REPO, "gdr_amd", "csrc", "gemm_f32.hip"), "rb") as f:
                    traffic_stale = tj.get("gemm_f32_sha16") != hashlib.sha256(f.read()).hexdigest()[:16]
            except Exception:
                traffic, traffic_stale = None, None
        peak = BF16_MFMA_PEAK_TFLOPS if (bf16 or form_terms) else F32_MFMA_PEAK_TFLOPS
        if form_terms:      # the 16-bit MFMA work really executed: (3 or 6 blocks) x the fp32-equivalent flops the profiler prices
            blocks = 3 if form_terms == 2 else form_terms
            lin["tflops"] *= blocks
            lin["gflop_per_launch"] *= blocks
        result = {
            "metric": "queries/sec on NQ-320k (768-d)", "value": total_q / dt, "unit": "queries/s",
            "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": ms_per_step,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": a.dtype if not form_terms else a.encoder_form, "data": "synthetic",
            "config": {"workload": ("C2" if world == 1 else "C4-layout") + ("/ragged" if ragged else "/padded") + ("/bf16" if bf16 else "") +
                       ("/prefilter" if use_pre else "") + (f"/{a.encoder_form}-linears(exploratory)" if form_terms else "") +
                       f": t5-base encoder {a.batch} q/GPU + Q.D^T top-{a.k}, {a.corpus}x{cfg.d_model} corpus",
                       "dist_backend": a.backend if dist.is_initialized() else None,
                       "batch_per_gpu": a.batch, "global_batch": a.batch * world, "seq_len": 40,
                       "corpus_rows": a.corpus, "dim": cfg.d_model, "k": a.k,
                       "encoder_rows": "ragged" if ragged else "padded", "live_token_rows_per_gpu": live_rows,
                       "corpus_setup_s": round(t_corpus, 2), "corpus_rows_on_host": int(D.shape[0])},
            "roofline": {"bound": "mfma",
                         "kernel": ("gdr::gemm_nt_bf16 (glds / persist256): every encoder linear" if bf16 else
                                    "gdr::gemm_nt_bf16_tile256_kernel<BN, split>: every encoder linear as 16-bit plane blocks" if form_terms else
                                    "gdr::gemm_nt_f32_persistent_kernel / gemm_nt_f32_streamk_kernel: every encoder linear"),
                         "achieved": lin["tflops"], "peak": peak, "unit": "TFLOP/s", "frac": lin["tflops"] / peak,
                         "traffic": None if (bf16 or form_terms) else traffic,
                         "traffic_source": None if (bf16 or form_terms or traffic is None) else "static: profiles/traffic.json (rocprofv3 --pmc passes of this command)",
                         "traffic_stale": None if (bf16 or form_terms or traffic is None) else bool(traffic_stale),
                         "launches": lin["launches"], "timed_steps": n_prof_steps, "avg_launch_ms": lin["avg_ms"],
                         "algorithmic_gflop_per_launch": lin["gflop_per_launch"], "share_of_step": lin["share_of_step"]},
        }
        detail = {"config_note": f"t5-base encoder on {a.batch} queries/GPU (L=40) + fused Q.D^T top-{a.k} over a "
                  f"{a.corpus}x{cfg.d_model} {'bf16' if bf16 else 'fp32'} corpus, resident in HBM" +
                  (" [C5 precision mode: bf16 linear operands, fp32 accumulate]" if bf16 else "") +
                  (f" [ragged encoder: the {live_rows} non-PAD token rows of {a.batch * 40} are computed, last block "
                   "on the CLS rows only; pooled output bit-identical to the padded form]" if ragged else
                   " [padded encoder: all batch x 40 rows]") +
                  ("" if world == 1 else f" row-sharded {world} ways, all-gather of queries, " +
                   ("one all-gather of the packed per-shard top-k, merge of all queries on every rank" if a.replicated_merge
                    else "one all-to-all of the packed per-shard top-k on a side stream under the next batch's encoder, "
                         "local merge")),
                  "roofline_sampling": f"hipEvent pairs around every dense launch of {n_prof_steps} of the {a.steps} timed steps (every "
                                       f"{max(1, a.prof_every)}th): `launches` counts the timed launches",
                  "roofline_note": "the same 128x128 MFMA K-step stream dealt as whole tiles or, where whole tiles quantise badly, as "
                                   "equal K-step ranges with exact accumulator hand-off; the last block's three CLS-row linears (64x64-tile "
                                   "kernel) are included in launches / flops / time",
                  "kernels": {"sim_sample_gemm": smp, "sim_filter_gemm": flt, "attention": att, "splitk_reduce": red}}
        if flt:
            # similarity as a whole (both GEMM passes): flops and the corpus bytes it must stream once
            sim_ms = (ms_l[1] + ms_l[2]) / n_prof_steps
            rows = hi - lo
            detail["kernels"]["sim_total"] = {
                "ms_per_step": sim_ms, "tflops": (w_l[1] + w_l[2]) / n_prof_steps / (sim_ms * 1e-3) / 1e12,
                "frac_of_mfma_peak": (w_l[1] + w_l[2]) / n_prof_steps / (sim_ms * 1e-3) / 1e12 /
                (BF16_MFMA_PEAK_TFLOPS if use_pre else peak),       # the corpus-wide passes run on the bf16 path then
                "corpus_stream_gbs": rows * cfg.d_model * (2 if bf16 else 4) / (sim_ms * 1e-3) / 1e9,
                "frac_of_hbm_peak": rows * cfg.d_model * (2 if bf16 else 4) / (sim_ms * 1e-3) / 1e9 / HBM_PEAK_GBS}
        # The CPU leg (rank 0, N = 1 only): the oracle timed on the host cores, and — the metric's second half —
        # Recall@{1,10,100} of the GPU top-k against the oracle's on the same synthetic queries, with every one of the
        # rows held to the top-k parity rule.  Nothing outside this leg touches oracle/.
        result["cpu_baseline"] = None
        result["recall"] = None
        if a.full and world == 1 and not a.no_cpu_baseline:
            if not a.no_recall:
                from oracle import retrieval_ref
                Q, gold = synth.make_queries(D, a.batch)
                gv, gi = ops.sim_topk(torch.from_numpy(Q).to(dev), D_dev, a.k)
                Dc = torch.from_numpy(D).to(torch.bfloat16).float() if bf16 else torch.from_numpy(D)
                Qc = torch.from_numpy(Q).to(torch.bfloat16).float() if bf16 else torch.from_numpy(Q)
                cv, ci = retrieval_ref.sim_topk(Qc, Dc, a.k, block=128)
                identical, permuted, bad = topk_parity(cv.numpy(), ci.numpy(), gv.cpu().numpy(), gi.cpu().numpy())
                result["recall"] = {"k": [1, 10, 100], "gpu": recall_at(gi.cpu().numpy(), gold),
                                    "cpu_oracle": recall_at(ci.numpy(), gold), "rows": a.batch,
                                    "topk_ids_identical_rows": identical, "permuted_slots": permuted,
                                    "rows_violating_tie_rule": bad}
                detail["recall_rule"] = ("values within 1e-4; ids exact outside groups of reference scores closer than 2e-4 "
                                         "(relative), same id set inside such a group")
                if pre is not None:   # the other similarity form against the same oracle lists, same rule
                    pv, pi = ops.sim_topk(torch.from_numpy(Q).to(dev), D_raw if use_pre else P, a.k)
                    pid, pperm, pbad = topk_parity(cv.numpy(), ci.numpy(), pv.cpu().numpy(), pi.cpu().numpy())
                    pre.update({"recall": recall_at(pi.cpu().numpy(), gold), "topk_ids_identical_rows": pid, "permuted_slots": pperm,
                                "rows_violating_tie_rule": pbad,
                                "rows_with_the_headline_path_ids": int((pi == gi).all(dim=1).sum().item())})
                    bad += pbad
                if bad:
                    emit(result, detail)
                    raise SystemExit(f"bench: {bad} rows differ from the CPU oracle outside tolerance-tie groups")
            result["cpu_baseline"] = cpu_baseline(sd, cfg, ids_all, mask_all, D, a.k)
        result["stages_summary"] = None
        if a.full and world == 1 and not a.no_stages and not bf16 and not form_terms:
            del enc
            if pre is not None:
                del P, index_p
                torch.cuda.empty_cache()
            detail["stages"] = stages(dev, cfg, D, D_raw, a)
            result["stages_summary"] = stages_summary(detail["stages"])
            if padded is not None:
                detail["stages"]["c2_step_padded"] = padded
                result["stages_summary"]["c2_padded_qps"] = padded["queries_per_s"]
                result["stages_summary"]["c2_padded_linear_frac"] = padded["linear_frac_of_f32_mfma_peak"]
            if split is not None:
                detail["stages"]["c2_step_split_bf16"] = split
                result["stages_summary"]["c2_split_bf16_qps"] = split["terms6"]["queries_per_s"]
                result["stages_summary"]["c2_split_bf16_tie_rule_violations"] = split["terms6"]["topk_vs_fp32_step"]["rows_violating_tie_rule"]
                result["stages_summary"]["c2_split3_16bit_qps"] = split["terms3"]["queries_per_s"]
                result["stages_summary"]["c2_split3_16bit_tie_rule_violations"] = split["terms3"]["topk_vs_fp32_step"]["rows_violating_tie_rule"]
                result["stages_summary"]["c2_split_f16x2_qps"] = split["f16x2"]["queries_per_s"]
                result["stages_summary"]["c2_split_f16x2_tie_rule_violations"] = split["f16x2"]["topk_vs_fp32_step"]["rows_violating_tie_rule"]
                result["stages_summary"]["c2_split_f16x2_pooled_max_abs_diff"] = split["f16x2"]["pooled_max_abs_diff_vs_fp32"]
            if pre is not None:
                # beside the headline, never instead of it: the same step with the other similarity form (same fp32 top-k for every
                # input; held to the same oracle lists by the same rule)
                beside = {"value": pre["queries_per_s"], "ms_per_step": pre["ms_per_step"], "recall": pre.get("recall"),
                          "rows_violating_tie_rule": pre.get("rows_violating_tie_rule"),
                          "topk_ids_identical_rows": pre.get("topk_ids_identical_rows")}
                note = ("gdr_sim_topk_prefilter: corpus-wide pass on the bf16 MFMA path over a bf16 image of the corpus, exact fp32 rescoring "
                        "of the docs inside the proven 2-eps band: the top-k of the fp32 scores for every input")
                if use_pre:
                    detail["stages"]["c2_step_all_fp32"] = pre
                    detail["stages"]["c2_step_bf16_prefilter_note"] = "the headline step runs " + note
                    result["all_fp32"] = beside
                    result["stages_summary"]["c2_all_fp32_qps"] = pre["queries_per_s"]
                    result["stages_summary"]["c2_prefilter_qps"] = result["value"]
                else:
                    detail["stages"]["c2_step_bf16_prefilter"] = pre
                    detail["stages"]["c2_step_bf16_prefilter_note"] = "the headline step with " + note
                    result["with_bf16_prefilter"] = beside
                    result["stages_summary"]["c2_prefilter_qps"] = pre["queries_per_s"]
        emit(result, detail if a.full else None)
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
