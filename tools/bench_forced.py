#!/usr/bin/env python3
"""The score mode of gdr_t5_generate (teacher-forced decode of given docid rows, ops.T5DecoderHandle.score) beside generate() of the
same shape, one GPU, one process.  Records numbers; sets no bar.

t5-base, random weights (no row ever emits EOS: a search runs all max_length - 1 = 9 decode steps), L = 40, on precomputed encoder
states, at 64 queries x 10 rows and 1 query x 100 rows: generate() (num_return_sequences = num_beams), then score() over the rows it
returned, without and with the hidden-state planes.  generate() is the yardstick because there is no earlier path to score given
rows; the mode runs one position more (max_length, the last one without a head) and none of the beam bookkeeping.  Every setting is
warmed up twice, then the settings are timed in turn, round after round (device event pairs around one call each), so that drift of
the machine falls on all of them alike; per setting the median and the spread (min, max) over the rounds, and the kernel launches
of one call (gdr_launch_count).

    python tools/bench_forced.py [--rounds 9] [--bf16] [--out FILE]

Prints one JSON line last.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES, MAXLEN, L, LP = ((64, 10), (1, 100)), 10, 40, 0.8


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
    settings, max_diff = {}, {}
    for B, R in SHAPES:
        ids, mask = synth.make_tokens(B, L=L, seed=21, min_len=8)
        ids, mask = torch.from_numpy(ids).to(dev), torch.from_numpy(mask).to(dev)
        enc_h, _ = enc.forward(ids, mask, want_pooled=False)
        rows, _lens, scores = dec.generate(enc_h, mask, R, MAXLEN, LP, R)
        max_diff[f"{B}x{R}"] = float((dec.score(enc_h, mask, rows, R, LP) - scores).abs().max())
        settings[f"{B}x{R}_generate"] = lambda e=enc_h, m=mask, R=R: dec.generate(e, m, R, MAXLEN, LP, R)
        settings[f"{B}x{R}_score"] = lambda e=enc_h, m=mask, R=R, r=rows: dec.score(e, m, r, R, LP)
        settings[f"{B}x{R}_score_hidden"] = lambda e=enc_h, m=mask, R=R, r=rows: dec.score(e, m, r, R, LP, hidden=True)
    launches = {}
    for name, fn in settings.items():
        fn(), fn()                                            # warm-up
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
    med = {n: float(np.median(t)) for n, t in times.items()}
    res = {"gpu": torch.cuda.get_device_name(0), "dtype": "bf16" if a.bf16 else "fp32", "L": L, "max_length": MAXLEN, "rounds": a.rounds,
           "ms": {n: {"median": round(med[n], 3), "min": round(min(t), 3), "max": round(max(t), 3)} for n, t in times.items()},
           "launches_per_call": launches,
           "score_over_generate": {f"{B}x{R}": round(med[f"{B}x{R}_score"] / med[f"{B}x{R}_generate"], 3) for B, R in SHAPES},
           "max_abs_score_difference_to_generate": max_diff}
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
