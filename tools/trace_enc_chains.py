#!/usr/bin/env python3
"""Encoder time budget of the C2 step from a rocprofv3 kernel trace of `bench.py --steps N --warmup W`: per step, the wall
time of the encoder call, the time in which at least one fp32 linear runs, the time in which only other encoder kernels
run, and the gaps; with two chains (GDR_ENC_CHAINS=2) also how long 0 / 1 / 2 linears run while both chains are alive.
A step's encoder call: from its first pack_len_kernel to the last kernel before sim_qprep_kernel.
usage: trace_enc_chains.py KERNEL_TRACE.csv [last_steps=5]"""
import csv, sys

rows = list(csv.DictReader(open(sys.argv[1])))
last = int(sys.argv[2]) if len(sys.argv) > 2 else 5
for r in rows:
    r["t0"], r["t1"] = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
rows.sort(key=lambda r: r["t0"])
name = lambda r: r["Kernel_Name"]
is_lin = lambda r: "gemm_nt_f32" in name(r)                      # every form of the fp32 linear, the CLS tail's small ones too
is_big = lambda r: is_lin(r) and "small" not in name(r) and int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"]) >= 192


def union(iv):
    tot, end, out = 0, None, []
    for a, b in sorted(iv):
        if end is None or a > end:
            out.append([a, b]); end = b
        elif b > end:
            out[-1][1] = b; end = b
    return out


def length(iv):
    return sum(b - a for a, b in iv)


def depth_hist(groups, lo, hi):
    """time in [lo, hi] during which exactly k of the interval groups are active"""
    ev = []
    for g in groups:
        for a, b in union(g):
            a, b = max(a, lo), min(b, hi)
            if b > a:
                ev += [(a, 1), (b, -1)]
    ev.sort()
    hist, d, t = [0] * (len(groups) + 1), 0, lo
    for x, s in ev:
        hist[d] += x - t; t = x; d += s
    hist[d] += hi - t
    return hist


ends = [i for i, r in enumerate(rows) if "sim_qprep_kernel" in name(r)]
steps = []
for e in ends:
    j = e - 1
    while j >= 0 and "sim_qprep_kernel" not in name(rows[j]):
        j -= 1
    seg = rows[j + 1:e]
    firsts = [i for i, r in enumerate(seg) if "pack_len_kernel" in name(r)]
    if firsts:
        steps.append(seg[firsts[0]:])
steps = steps[-last:]
acc = {}
def add(k, v):
    acc.setdefault(k, []).append(v)
for seg in steps:
    lo, hi = seg[0]["t0"], max(r["t1"] for r in seg)
    lin = union([(r["t0"], r["t1"]) for r in seg if is_lin(r)])
    anyk = union([(r["t0"], r["t1"]) for r in seg])
    add("encoder wall", hi - lo)
    add("a linear running", length(lin))
    add("only other kernels", length(anyk) - length(lin))
    add("gaps", hi - lo - length(anyk))
    add("sum of linear durations", sum(r["t1"] - r["t0"] for r in seg if is_lin(r)))
    add("sum of other durations", sum(r["t1"] - r["t0"] for r in seg if not is_lin(r)))
    add("launches", len(seg))
    chains = sorted({r["Stream_Id"] + "/" + r["Queue_Id"] for r in seg if is_big(r)})
    if len(chains) == 2:
        per = [[(r["t0"], r["t1"]) for r in seg if is_big(r) and r["Stream_Id"] + "/" + r["Queue_Id"] == c] for c in chains]
        alive = [(min(r["t0"] for r in seg if r["Stream_Id"] + "/" + r["Queue_Id"] == c),
                  max(r["t1"] for r in seg if r["Stream_Id"] + "/" + r["Queue_Id"] == c)) for c in chains]
        a, b = max(x[0] for x in alive), min(x[1] for x in alive)
        h = depth_hist(per, a, b)
        add("both chains alive", b - a)
        add("  0 big linears (both chains in a boundary)", h[0])
        add("  1 big linear", h[1])
        add("  2 big linears", h[2])
print(f"{len(steps)} steps, mean per step (us):")
for k, v in acc.items():
    m = sum(v) / len(v)
    print(f"  {k:46s} {m if k == 'launches' else m / 1e3:10.1f}")
w = sum(acc["encoder wall"]) / len(steps)
print(f"  fraction of the encoder's wall time with a linear running: {sum(acc['a linear running']) / len(steps) / w:.4f}")
