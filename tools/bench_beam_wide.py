#!/usr/bin/env python3
"""The beam decode at 100, 300 and 1024 beams, one GPU (DESIGN.md §4 "Beam decode beyond 8192 candidates").  Records numbers; sets no bar.

V = 30, 64 queries, max_length = 10 (9 decode steps).  Per build and setting, in a fresh process each (the library and the switch
GDR_DECODE_BEAM_CHUNKED are fixed at load time):
  * the beam machinery alone — gdr_beam_search_table on a random logit table: table look-up + top-2R select + bookkeeping per step —
    as us per step (median of event pairs over whole calls after two warm-up calls, divided by the 9 steps) and launches per step;
  * generate() of t5-base on precomputed encoder states (L = 40): ms per call.
100 beams run the one-sort kernel in every build; 300 and 1024 beams need this revision (an older build refuses them: null).

    python tools/bench_beam_wide.py [--reps 7] [--queries 64] [--parent-lib OLD/libgdr_hip.so] [--out FILE]

With --parent-lib the old and the new build are timed alternately (old, new, old, new forced-chunked): the spread of the two old
runs is the noise floor under which a difference between old and new at 100 beams means nothing.  Prints one JSON line last.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BEAMS, V, MAXLEN, L = (100, 300, 1024), 30, 10, 40


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


def child(a):
    import torch
    from gdr_amd import _ffi, ops, synth
    from gdr_amd.config import GDRConfig
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    B, steps = a.queries, MAXLEN - 1
    res = {"lib": os.environ.get("GDR_HIP_LIB", "default"), "chunked": os.environ.get("GDR_DECODE_BEAM_CHUNKED", "0"),
           "gpu": torch.cuda.get_device_name(0), "queries": B, "table_us_per_step": {}, "table_launches_per_step": {},
           "generate_ms": {}}
    Vd = V * MAXLEN + 2
    g = torch.Generator(device="cpu").manual_seed(7)
    table = torch.randn((B, MAXLEN, Vd, Vd), generator=g).to(dev)
    for R in BEAMS:
        try:
            ms = timed_dev(lambda: ops.beam_search_table(table, V, R, MAXLEN, 0.8), a.reps)
            n0 = _ffi.lib().gdr_launch_count()
            ops.beam_search_table(table, V, R, MAXLEN, 0.8)
            res["table_launches_per_step"][str(R)] = round((_ffi.lib().gdr_launch_count() - n0 - 2) / steps, 2)   # - init, finalize
            res["table_us_per_step"][str(R)] = round(ms * 1e3 / steps, 1)
        except _ffi.GdrError as e:
            res["table_us_per_step"][str(R)] = None
            res.setdefault("refused", {})[str(R)] = str(e)[:120]
        print("table", R, res["table_us_per_step"][str(R)], flush=True)
    del table
    if not a.no_generate:
        cfg = GDRConfig.base()
        sd = synth.make_state_dict(cfg, seed=1234)
        enc, dec = ops.T5EncoderHandle(cfg, sd, dev), ops.T5DecoderHandle(cfg, sd, dev)
        ids, mask = synth.make_tokens(B, L=L, seed=21, min_len=8)
        ids, mask = torch.from_numpy(ids).to(dev), torch.from_numpy(mask).to(dev)
        enc_h, _ = enc.forward(ids, mask, want_pooled=False)
        for R in BEAMS:
            try:
                ms = timed_dev(lambda: dec.generate(enc_h, mask, R, MAXLEN, 0.8, R), max(3, a.reps // 2))
                res["generate_ms"][str(R)] = round(ms, 3)
            except (_ffi.GdrError, torch.OutOfMemoryError) as e:
                res["generate_ms"][str(R)] = None
                res.setdefault("refused", {})[f"generate_{R}"] = str(e)[:120]
            print("generate", R, res["generate_ms"][str(R)], flush=True)
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--parent-lib", default=None, help="libgdr_hip.so of the build to compare with")
    ap.add_argument("--no-generate", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    runs = [("new", None, "0")]
    if a.parent_lib:
        runs = [("parent_1", a.parent_lib, "0"), ("new", None, "0"), ("parent_2", a.parent_lib, "0")]
    runs.append(("new_forced_chunked", None, "1"))
    out = {}
    for name, lib, chunked in runs:       # one process at a time; the first one that fails ends the run
        env = dict(os.environ, GDR_DECODE_BEAM_CHUNKED=chunked)
        env.pop("GDR_HIP_LIB", None)
        if lib:
            env["GDR_HIP_LIB"] = os.path.abspath(lib)
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--queries", str(a.queries)]
        if a.no_generate:
            cmd.append("--no-generate")
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            print(r.stdout[-2000:], r.stderr[-2000:], file=sys.stderr)
            sys.exit(f"{name}: exit status {r.returncode}")
        out[name] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
        print(name, json.dumps(out[name]), flush=True)
    if a.parent_lib:
        floor = {}
        for key in ("table_us_per_step", "generate_ms"):
            p1, p2 = out["parent_1"][key].get("100"), out["parent_2"][key].get("100")
            if p1 and p2:
                floor[key] = {"parent_spread": round(abs(p1 - p2), 3), "new_minus_parent_mean": round(out["new"][key]["100"] - (p1 + p2) / 2, 3)}
        out["at_100_beams"] = floor
    line = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
