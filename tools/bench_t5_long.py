#!/usr/bin/env python3
"""The T5 query tower and generate() at up to 512 input tokens, one process, one GPU.  Records numbers; sets no bar.

t5-base, full-length inputs.  Encoder at equal token counts — 512 x 40 and 256 x 128 (the one-pass attention kernels), 64 x 512 (the
key-block kernel with position bias of csrc/attention_long.hip) — in the padded fp32, ragged fp32 and ragged bf16 forms: ms (median of
event pairs after two warm-up calls) and tokens/s.  generate() at 64 queries x 10 beams with L = 40, 128 and 512 on precomputed
encoder states: ms per call.  Prints one JSON line last.

    python tools/bench_t5_long.py [--reps 7] [--out FILE]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_t5_long.py --reps 3
    python tools/bench_t5_long.py --stats DIR/.../*_kernel_stats.csv     # attention kernels of that trace: calls, mean / max us (no GPU)
    python tools/bench_t5_long.py --digest   # sha1 of every encoder form's outputs and of generate()'s ids and scores at L = 40 and
                                             # L = 128: compare two builds (GDR_HIP_LIB)
"""
import argparse
import csv
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FORMS = (("padded_f32", "f32", False), ("ragged_f32", "f32", True), ("ragged_bf16", "bf16", True))
SHAPES = ((512, 40), (256, 128), (64, 512))
GEN_B, GEN_R = 64, 10


def handles(dev, seed=1234):
    import torch
    from gdr_amd import ops, synth
    from gdr_amd.config import GDRConfig
    cfg = GDRConfig.base()
    sd = synth.make_state_dict(cfg, seed=seed)
    enc = {"f32": ops.T5EncoderHandle(cfg, sd, dev), "bf16": ops.T5EncoderHandle(cfg, sd, dev, dtype=torch.bfloat16)}
    return cfg, sd, enc


def timed_dev(fn, reps):
    """median ms between device events around fn(), after two warm-up calls."""
    import torch
    fn(), fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def bench(a):
    import torch
    from gdr_amd import ops
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    cfg, sd, enc = handles(dev)
    res = {"gpu": torch.cuda.get_device_name(0), "gpus": 1, "reps": a.reps, "encoder": {}, "generate": {}}
    g = np.random.Generator(np.random.PCG64(3))
    for name, prec, ragged in FORMS:
        row = {}
        for B, L in SHAPES:
            ids = torch.from_numpy(g.integers(2, 32100, size=(B, L)).astype(np.int64)).to(dev)
            mask = torch.ones_like(ids)
            ms = timed_dev(lambda: enc[prec].forward(ids, mask, ragged=ragged, live_rows_hint=B * L if ragged else -1), a.reps)
            row[f"{B}x{L}"] = {"ms": round(ms, 3), "tokens_per_s": round(B * L / ms * 1e3)}
        res["encoder"][name] = row
        print(name, json.dumps(row), flush=True)
    dec = ops.T5DecoderHandle(cfg, sd, dev)
    for L in (40, 128, 512):
        ids = torch.from_numpy(g.integers(2, 32100, size=(GEN_B, L)).astype(np.int64)).to(dev)
        mask = torch.ones_like(ids)
        enc_h, _ = enc["f32"].forward(ids, mask, want_pooled=False)
        ms = timed_dev(lambda: dec.generate(enc_h, mask, GEN_R, cfg.max_output_length, 0.8, GEN_R), a.reps)
        res["generate"][f"{GEN_B}x{GEN_R}_L{L}"] = {"ms": round(ms, 3)}
        print("generate", L, round(ms, 3), flush=True)
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


def stats(a):
    """The attention kernels of one rocprofv3 kernel_stats.csv: calls, mean and longest launch."""
    out = {}
    with open(a.stats) as f:
        for r in csv.DictReader(f):
            if "attention" in r["Name"]:
                out[r["Name"].split("(")[0]] = {"calls": int(r["Calls"]), "mean_us": round(float(r["AverageNs"]) / 1e3, 2),
                                               "max_us": round(float(r["MaxNs"]) / 1e3, 2), "percent": float(r["Percentage"])}
    print(json.dumps(out))


def digest(a):
    """sha1 of pooled / hidden / pooled-only outputs of every encoder form and of generate()'s ids and scores at L = 40 and L = 128 on
    seeded inputs: equal between two builds means the L <= 128 routing and arithmetic did not change."""
    import torch
    from gdr_amd import ops, synth
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    cfg, sd, enc = handles(dev)
    dec = {"f32": ops.T5DecoderHandle(cfg, sd, dev), "bf16": ops.T5DecoderHandle(cfg, sd, dev, dtype=torch.bfloat16)}
    esp = {split: ops.T5EncoderHandle(cfg, sd, dev, split=split) for split in (6, 2)}
    sha = lambda t: hashlib.sha1(t.cpu().numpy().tobytes()).hexdigest()[:16]
    out = {}
    for L in (40, 128):
        ids_n, mask_n = synth.make_tokens(48, L=L, seed=9, min_len=8)
        ids, mask = torch.from_numpy(ids_n).to(dev), torch.from_numpy(mask_n).to(dev)
        for name, prec, ragged in FORMS + (("padded_bf16", "bf16", False),):
            hid, pooled = enc[prec].forward(ids, mask, ragged=ragged)
            _, ponly = enc[prec].forward(ids, mask, ragged=ragged, want_hidden=False)
            out[f"L{L}_{name}"] = [sha(pooled), sha(hid), sha(ponly)]
        for split in (6, 2):
            hid, pooled = esp[split].forward(ids, mask, ragged=True)
            _, ponly = esp[split].forward(ids, mask, ragged=True, want_hidden=False)
            out[f"L{L}_split{split}"] = [sha(pooled), sha(hid), sha(ponly)]
        for prec in ("f32", "bf16"):
            enc_h, _ = enc[prec].forward(ids[:16], mask[:16], want_pooled=False)
            o_ids, lens, scores = dec[prec].generate(enc_h, mask[:16], GEN_R, cfg.max_output_length, 0.8, GEN_R)[:3]
            out[f"L{L}_generate_{prec}"] = [sha(o_ids), sha(scores)]
    print(json.dumps({"lib": os.environ.get("GDR_HIP_LIB", "default"), "digest": out}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--stats", default=None)
    ap.add_argument("--digest", action="store_true")
    a = ap.parse_args()
    if a.stats:
        return stats(a)
    if a.digest:
        return digest(a)
    return bench(a)


if __name__ == "__main__":
    main()
