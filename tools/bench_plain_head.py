#!/usr/bin/env python3
"""generate() of the adaptor-free model (plain lm_head docid head) beside the adaptor model, one GPU, one process (DESIGN.md §4
"Plain lm_head docid head").  Records numbers; sets no bar.

t5-base, random weights (no row ever emits EOS: all max_length - 1 = 9 decode steps run), L = 40, on precomputed encoder states:
gdr_t5_generate for the adaptor model and the plain model at 64 x 10, 512 x 10, 512 x 30, 1 x 100 and 64 x 1 (queries x beams), as host
launches and as a replayed graph.  Every setting is warmed up twice, then the settings are timed in turn — adaptor, plain, adaptor, ... —
round after round (device event pairs around one call each), so that drift of the machine falls on all of them alike; per setting the
median and the spread (min, max) over the rounds, the kernel launches of one call, the workspace bytes of both models and the bytes
the decoder handles keep resident.

    python tools/bench_plain_head.py [--rounds 9] [--bf16] [--shapes 64x10,512x10] [--out FILE]

Prints one JSON line last.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES, MAXLEN, L = "64x10,512x10,512x30,1x100,64x1", 10, 40


def resident_bytes(handle):
    seen, total = set(), 0
    for t in list(handle._keep) + [handle.head_e, handle.head_w]:
        if t is not None and t.data_ptr() not in seen:
            seen.add(t.data_ptr())
            total += t.numel() * t.element_size()
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--bf16", action="store_true", help="the bf16 precision mode instead of fp32")
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from gdr_amd import _ffi, ops, synth
    from gdr_amd.config import GDRConfig
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    dtype = torch.bfloat16 if a.bf16 else torch.float32
    cfg = GDRConfig.base()
    sd = synth.make_state_dict(cfg, seed=1234)
    enc = ops.T5EncoderHandle(cfg, sd, dev, dtype=dtype)
    models = {"adaptor": ops.T5DecoderHandle(cfg, sd, dev, dtype=dtype)}
    plain_cfg = GDRConfig.base(adaptor_decode=0, adaptor_efficient=0)
    models["plain"] = ops.T5DecoderHandle(plain_cfg, {k: v for k, v in sd.items() if not k.startswith("adaptor")}, dev, dtype=dtype)
    del sd
    shapes = [tuple(int(x) for x in s.split("x")) for s in a.shapes.split(",")]
    settings, workspace = {}, {}
    for B, R in shapes:
        ids, mask = synth.make_tokens(B, L=L, seed=21, min_len=8)
        ids, mask = torch.from_numpy(ids).to(dev), torch.from_numpy(mask).to(dev)
        enc_h, _ = enc.forward(ids, mask, want_pooled=False)
        for graph in (False, True):
            for which, dec in models.items():                  # adaptor and plain alternate inside a round
                settings[f"{B}x{R}_{which}" + ("_graph" if graph else "")] = (
                    lambda e=enc_h, m=mask, R=R, g=graph, d=dec: d.generate(e, m, R, MAXLEN, 0.8, R, graph=g))
        workspace[f"{B}x{R}"] = {w: int(_ffi.lib().gdr_t5_generate_workspace_bytes(C.byref(d.struct), B, L, R, MAXLEN))
                                 for w, d in models.items()}
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
           "launches_per_call": launches, "workspace_bytes": workspace,
           "handle_resident_bytes": {w: resident_bytes(d) for w, d in models.items()}}
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
