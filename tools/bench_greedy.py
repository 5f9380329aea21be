#!/usr/bin/env python3
"""generate() at num_beams = 1 (greedy decode) beside 2 and 10 beams, one GPU, one process (DESIGN.md §4 "Greedy decode").  Records
numbers; sets no bar.

t5-base, random weights (no row ever emits EOS: all max_length - 1 = 9 decode steps run), L = 40, on precomputed encoder states:
gdr_t5_generate for 64 and 512 queries at 1, 2 and 10 beams, as host launches and as a replayed graph.  Every setting is warmed up
twice, then the settings are timed in turn, round after round (device event pairs around one call each), so that drift of the machine
falls on all of them alike; per setting the median and the spread (min, max) over the rounds, and the kernel launches of one call.

    python tools/bench_greedy.py [--rounds 9] [--out FILE]

Prints one JSON line last.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
QUERIES, BEAMS, MAXLEN, L = (64, 512), (1, 2, 10), 10, 40


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--bf16", action="store_true", help="the bf16 precision mode instead of fp32")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from gdr_amd import _ffi, ops, synth
    from gdr_amd.config import GDRConfig
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    cfg = GDRConfig.base()
    sd = synth.make_state_dict(cfg, seed=1234)
    dtype = torch.bfloat16 if a.bf16 else torch.float32
    enc, dec = ops.T5EncoderHandle(cfg, sd, dev, dtype=dtype), ops.T5DecoderHandle(cfg, sd, dev, dtype=dtype)
    settings = {}
    for B in QUERIES:
        ids, mask = synth.make_tokens(B, L=L, seed=21, min_len=8)
        ids, mask = torch.from_numpy(ids).to(dev), torch.from_numpy(mask).to(dev)
        enc_h, _ = enc.forward(ids, mask, want_pooled=False)
        for R in BEAMS:
            for graph in (False, True):
                settings[f"{B}x{R}" + ("_graph" if graph else "")] = (
                    lambda e=enc_h, m=mask, R=R, g=graph: dec.generate(e, m, R, MAXLEN, 0.8, R, graph=g))
    launches = {}
    for name, fn in settings.items():
        fn(), fn()                                            # warm-up (a graph setting: capture, then one replay)
        if not name.endswith("_graph"):
            n0 = _ffi.lib().gdr_launch_count()
            fn()
            launches[name] = int(_ffi.lib().gdr_launch_count() - n0)
    torch.cuda.synchronize()
    times = {name: [] for name in settings}
    for _ in range(a.rounds):
        for name, fn in settings.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            times[name].append(t0.elapsed_time(t1))
    res = {"gpu": torch.cuda.get_device_name(0), "dtype": "bf16" if a.bf16 else "fp32", "L": L, "max_length": MAXLEN, "rounds": a.rounds,
           "ms": {n: {"median": round(float(np.median(t)), 3), "min": round(min(t), 3), "max": round(max(t), 3)} for n, t in times.items()},
           "launches_per_call": launches}
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
