#!/usr/bin/env python3
"""Document removal at the C2 index size: 320,000 members in the 26,667 clusters of 12 of synth's default index
(members shuffled inside every cluster), 1,000 random ids removed.

Reports, each the median of --reps runs in this one process after a warm-up:
  * ops.DeviceClusterIndex.remove end to end (host clock around a device synchronise): the ascending check of the id list, the
    three launches of gdr_cluster_insert's removal mode, one read-back of (new total, largest cluster), the struct rebuild;
  * the three launches alone (device events around the raw call);
  * a torch restatement of the same compaction (isin + boolean mask + cumsum, one read-back of the largest cluster), host clock
    and device events likewise.  Its result is compared with the kernel's before anything is timed.
Prints one JSON line last.

    python tools/bench_lifecycle.py [--members 320000] [--remove 1000] [--reps 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gdr_amd import codec, ops, synth                     # noqa: E402
from gdr_amd._ffi import check, lib, ptr, stream_ptr     # noqa: E402


def timed(fn, reps, before=None):
    """median ms of fn() by the host clock, device work included; before() (untimed) restores the state fn() consumes."""
    ts = []
    for i in range(reps + 1):                             # run 0 is the warm-up
        if before:
            before()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts[1:]))


def timed_dev(fn, reps):
    """median ms between device events around fn()."""
    fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def torch_remove(offs, mem, ids):
    """The same compaction in torch: (offsets int32[C+1], members, largest cluster)."""
    keep = ~torch.isin(mem, ids)
    before = torch.cumsum(keep, 0, dtype=torch.int32)
    new_off = torch.cat([before.new_zeros(1), before])[offs.long()]
    out = mem[keep]
    return new_off, out, int((new_off[1:] - new_off[:-1]).max().item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=320000)
    ap.add_argument("--remove", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    N, csz, V = a.members, 12, 30
    rng = np.random.default_rng(0)
    n_cl = (N + csz - 1) // csz
    offs = np.minimum(np.arange(n_cl + 1, dtype=np.int64) * csz, N).astype(np.int32)
    mem = np.concatenate([rng.permutation(np.arange(offs[c], offs[c + 1])) for c in range(n_cl)]).astype(np.int32)
    names = ["-".join(str(x) for x in synth.cluster_digits(c, 4, V)) for c in range(n_cl)]
    dci = ops.DeviceClusterIndex(codec.ClusterIndex(names, offs, mem), dev, V, position=1, kary=V)
    ids = torch.from_numpy(np.sort(rng.choice(N, a.remove, replace=False)).astype(np.int32)).to(dev)
    offs_d, mem_d = dci.offsets, dci.members

    o, m, mx, gone = ops.cluster_remove(offs_d, mem_d, ids)
    to, tm, tmx = torch_remove(offs_d, mem_d, ids)
    assert torch.equal(o, to) and torch.equal(m, tm) and mx == tmx and gone == a.remove, "the torch form disagrees with the kernel"

    def restore():
        dci.offsets, dci.members, dci.n_members, dci.max_cluster = offs_d, mem_d, N, csz
    t_remove = timed(lambda: dci.remove(ids), a.reps, before=restore)
    restore()
    need = lib().gdr_cluster_insert_workspace_bytes(n_cl)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out_off = torch.empty(n_cl + 1, dtype=torch.int32, device=dev)
    out_mem = torch.empty(N, dtype=torch.int32, device=dev)
    out_max = torch.empty(1, dtype=torch.int32, device=dev)
    raw = lambda: check(lib().gdr_cluster_insert(ptr(offs_d), ptr(mem_d), n_cl, N, ptr(ids), None, a.remove, None, 0, ptr(out_off),   # noqa: E731
                                                 ptr(out_mem), ptr(out_max), ptr(ws), need, stream_ptr()), "gdr_cluster_insert")
    t_kernels = timed_dev(raw, a.reps)
    t_torch = timed(lambda: torch_remove(offs_d, mem_d, ids), a.reps)
    t_torch_dev = timed_dev(lambda: torch_remove(offs_d, mem_d, ids), a.reps)

    print(f"index: {N} members in {n_cl} clusters of {csz}; {a.remove} ids removed; median of {a.reps}")
    print(f"DeviceClusterIndex.remove   {t_remove * 1e3:9.1f} us   (host clock, read-backs included)")
    print(f"  its three launches        {t_kernels * 1e3:9.1f} us   (device events)")
    print(f"torch isin + mask + cumsum  {t_torch * 1e3:9.1f} us   (host clock, read-back included)")
    print(f"  between device events     {t_torch_dev * 1e3:9.1f} us")
    print(json.dumps({"bench": "lifecycle", "members": N, "clusters": n_cl, "removed": a.remove, "reps": a.reps,
                      "remove_us": round(t_remove * 1e3, 1), "remove_kernels_us": round(t_kernels * 1e3, 1),
                      "torch_us": round(t_torch * 1e3, 1), "torch_device_us": round(t_torch_dev * 1e3, 1),
                      "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
