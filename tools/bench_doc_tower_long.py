#!/usr/bin/env python3
"""The doc tower at 512 tokens against the doc tower at 128 tokens, equal token counts, one process.

bert-base, full-length passages: 256 x 128 (the one-pass attention kernels) and 64 x 512 (the key-block kernels of
csrc/attention_long.hip) for the padded fp32, ragged fp32, ragged bf16 and split (fp16 x 2) forms: ms (median of event pairs after
warm-up) and tokens/s, the measured tokens/s ratio 512 : 128 beside the ideal 0.925 from the flop counts (per token 14.2 MFLOP of
linears at any length, 4 * L * 768 of attention).  Plus a ragged case with a reference-like length mix (make_tokens(64, L=512,
min_len=100)): ms and live tokens/s.  One GPU; nothing here was measured on more than one.  Prints one JSON line last.

    python tools/bench_doc_tower_long.py [--reps 7] [--out FILE]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_doc_tower_long.py --reps 3 --no-mix
    python tools/bench_doc_tower_long.py --stats DIR/.../*_kernel_stats.csv --bench FILE     # attention rates and shares (no GPU)
    python tools/bench_doc_tower_long.py --digest    # sha1 of the tower's outputs at L = 40 and 128: compare two builds (GDR_HIP_LIB)
    python tools/bench_doc_tower_long.py --rows-check   # 256 x 512 = 131 072 rows in one call equal four calls of 64 x 512
"""
import argparse
import csv
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FORMS = (("padded_f32", dict(ragged=False)), ("ragged_f32", dict(ragged=True)), ("ragged_bf16", dict(dtype="bf16")),
         ("split_f16x2", dict(split=True)))
H, DKV, LAYERS = 12, 64, 12


def towers(dev, seed=77):
    import torch
    from gdr_amd import synth
    from gdr_amd.modeling import EncoderModel
    bc = synth.bert_config(False)
    sd = synth.make_bert_state_dict(bc, seed=seed)
    out = {}
    for name, kw in FORMS:
        kw = dict(kw)
        if kw.pop("dtype", None) == "bf16":
            kw["dtype"] = torch.bfloat16
        out[name] = EncoderModel.from_state_dict(bc, sd, dev, **kw)
    return bc, out


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
    from gdr_amd import synth
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    bc, tw = towers(dev)
    res = {"gpu": torch.cuda.get_device_name(0), "gpus": 1, "reps": a.reps, "forms": {}}
    g = np.random.Generator(np.random.PCG64(3))
    for name, _ in FORMS:
        row = {}
        for B, L in ((256, 128), (64, 512)):
            ids = torch.from_numpy(g.integers(2, bc["vocab_size"], size=(B, L)).astype(np.int64)).to(dev)
            mask = torch.ones_like(ids)
            ms = timed_dev(lambda: tw[name](passage={"input_ids": ids, "attention_mask": mask}), a.reps)
            row[f"{B}x{L}"] = {"ms": round(ms, 3), "tokens_per_s": round(B * L / ms * 1e3)}
        row["tokens_per_s_ratio_512_to_128"] = round(row["64x512"]["tokens_per_s"] / row["256x128"]["tokens_per_s"], 4)
        res["forms"][name] = row
        print(name, json.dumps(row), flush=True)
    res["ideal_ratio_from_flops"] = round((14.2 + 4 * 128 * 768 / 1e6) / (14.2 + 4 * 512 * 768 / 1e6), 4)
    ids_n, mask_n = synth.make_tokens(64, L=512, vocab_hi=bc["vocab_size"], seed=5, min_len=100)
    ids, mask = torch.from_numpy(ids_n).to(dev), torch.from_numpy(mask_n).to(dev)
    live = int(mask_n.sum())
    res["ragged_mix_64x512"] = {"live_tokens": live}
    for name in () if a.no_mix else ("ragged_f32", "ragged_bf16", "split_f16x2"):
        ms = timed_dev(lambda: tw[name](passage={"input_ids": ids, "attention_mask": mask}), a.reps)
        res["ragged_mix_64x512"][name] = {"ms": round(ms, 3), "live_tokens_per_s": round(live / ms * 1e3)}
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


def stats(a):
    """Attention kernel rates from a rocprofv3 kernel_stats.csv of one bench run: 4 * B * H * L^2 * d_kv flops over the mean time, the
    key-block kernels at 64 x 512 against the one-pass kernels at 256 x 128 in the same trace, and the attention share of each form."""
    mean = {}
    with open(a.stats) as f:
        for r in csv.DictReader(f):
            for key in ("attention_mfma16_kernel<8>", "attention_mfma_bf16_kernel<8>", "attention_long_f32_kernel", "attention_long_bf16_kernel"):
                if key in r["Name"]:
                    mean[key] = (float(r["AverageNs"]), int(r["Calls"]))
    fl = {128: 4.0 * 256 * H * 128 * 128 * DKV, 512: 4.0 * 64 * H * 512 * 512 * DKV}
    out = {}
    for prec, k128, k512 in (("f32", "attention_mfma16_kernel<8>", "attention_long_f32_kernel"),
                             ("bf16", "attention_mfma_bf16_kernel<8>", "attention_long_bf16_kernel")):
        r128, r512 = fl[128] / mean[k128][0] / 1e3, fl[512] / mean[k512][0] / 1e3      # TFLOP/s
        out[prec] = {"one_pass_256x128": {"mean_us": round(mean[k128][0] / 1e3, 2), "calls": mean[k128][1], "tflops": round(r128, 2)},
                     "key_block_64x512": {"mean_us": round(mean[k512][0] / 1e3, 2), "calls": mean[k512][1], "tflops": round(r512, 2)},
                     "rate_ratio": round(r512 / r128, 3), "bar": 0.8}
    if a.bench:
        with open(a.bench) as f:
            b = json.loads(f.read().strip().splitlines()[-1])
        share = {}
        for name, _ in FORMS:
            p = "bf16" if "bf16" in name else "f32"
            share[name] = {"256x128": round(LAYERS * out[p]["one_pass_256x128"]["mean_us"] / 1e3 / b["forms"][name]["256x128"]["ms"], 4),
                           "64x512": round(LAYERS * out[p]["key_block_64x512"]["mean_us"] / 1e3 / b["forms"][name]["64x512"]["ms"], 4)}
        out["attention_share_of_forward"] = share
    print(json.dumps(out))


def digest(a):
    """sha1 of pooled and hidden outputs at L = 40 and L = 128 on seeded inputs, every form: equal between two builds means the
    L <= 128 routing and arithmetic did not change."""
    import torch
    from gdr_amd import synth
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    bc, tw = towers(dev)
    out = {}
    for L in (40, 128):
        ids_n, mask_n = synth.make_tokens(48, L=L, vocab_hi=bc["vocab_size"], seed=9, min_len=8)
        ids, mask = torch.from_numpy(ids_n).to(dev), torch.from_numpy(mask_n).to(dev)
        for name, kw in FORMS:
            hid, pooled = tw[name].bert.forward(ids, mask, ragged=kw.get("ragged"))
            _, ponly = tw[name].bert.forward(ids, mask, ragged=kw.get("ragged"), want_hidden=False)
            out[f"L{L}_{name}"] = [hashlib.sha1(t.cpu().numpy().tobytes()).hexdigest()[:16] for t in (pooled, hid, ponly)]
    print(json.dumps({"lib": os.environ.get("GDR_HIP_LIB", "default"), "digest": out}))


def rows_check(a):
    import torch
    from gdr_amd import synth
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    bc, tw = towers(dev)
    ids_n, mask_n = synth.make_tokens(256, L=512, vocab_hi=bc["vocab_size"], seed=31, min_len=400)
    mask_n[:4, :] = 1
    ids, mask = torch.from_numpy(ids_n).to(dev), torch.from_numpy(mask_n).to(dev)
    res = {"rows": int(ids.numel())}
    for name, _ in FORMS:
        whole = tw[name](passage={"input_ids": ids, "attention_mask": mask})
        parts = torch.cat([tw[name](passage={"input_ids": ids[i:i + 64], "attention_mask": mask[i:i + 64]}) for i in range(0, 256, 64)])
        res[name] = {"finite": bool(torch.isfinite(whole).all()), "max_abs_diff_vs_4x64": float((whole - parts).abs().max())}
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--stats", default=None)
    ap.add_argument("--bench", default=None)
    ap.add_argument("--digest", action="store_true")
    ap.add_argument("--rows-check", action="store_true")
    ap.add_argument("--no-mix", action="store_true", help="full-length passages only: under a kernel trace every launch of a kernel is "
                                                          "then the same work and its mean time is the time of that work")
    a = ap.parse_args()
    if a.stats:
        return stats(a)
    if a.digest:
        return digest(a)
    if a.rows_check:
        return rows_check(a)
    return bench(a)


if __name__ == "__main__":
    main()
