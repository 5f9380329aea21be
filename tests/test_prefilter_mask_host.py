"""The pre-filtered search over live rows / per-query filters, host side: the exported symbols and their prototypes,
the workspace sizing and the pre-launch refusals of gdr_sim_topk_prefilter_masked, the refusals of gdr_prefilter_update_rows, the
routing predicate of ops.sim_topk over a PrefilteredCorpus (with stubs), and the numpy restatement of the plan that
tests/test_gpu_prefilter_mask.py uses to show that its cases cannot flag.  Needs no GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import test_gpu_prefilter_mask as gpu
from conftest import REPO
from gdr_amd import _ffi, ops

LIVE, QM = _ffi.SIM_LIVE_MASK, _ffi.SIM_QUERY_MASK
SIZES = [(8, 70_001, 128, 10), (512, 320_000, 768, 100), (4, 1000, 64, 10), (40, 20_000, 64, 10), (4, 20_011, 256, 10), (40, 20_000, 64, 100),
         (40, 2_800_003, 768, 1024)]
CTYPE = {"size_t": C.c_size_t, "int": C.c_int, "int64_t": C.c_int64, "int32_t": C.c_int32, "float": C.c_float}


def _header():
    text = open(os.path.join(REPO, "include", "gdr_hip_prefilter_mask.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return {m.group(2): (m.group(1), " ".join(m.group(3).split()))
            for m in re.finditer(r"\b(size_t|int)\s+(gdr_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S)}


def test_symbols_are_exported_and_the_header_prototypes_match_the_binding():
    protos = _header()
    assert set(protos) == set(_ffi.PREFILTER_MASK_SIGNATURES) == {"gdr_sim_topk_prefilter_masked_workspace_bytes", "gdr_sim_topk_prefilter_masked",
                                                                  "gdr_prefilter_update_rows"}
    assert not set(_ffi.PREFILTER_MASK_SIGNATURES) & set(_ffi.SIGNATURES)
    l = _ffi.lib()
    for name, (ret, params) in protos.items():
        fn = getattr(l, name)                                                  # AttributeError: the library does not export it
        res, args = _ffi.PREFILTER_MASK_SIGNATURES[name]
        assert fn.restype is res is CTYPE[ret] and fn.argtypes == args
        want = [C.c_void_p if "*" in p else CTYPE[p.split()[-2]] for p in params.split(",")]
        assert args == want, (name, params)
    assert l.gdr_abi_version() == 9 == _ffi.ABI_VERSION
    main = open(os.path.join(REPO, "include", "gdr_hip.h")).read()
    assert '#include "gdr_hip_prefilter_mask.h"' in main, "gdr_hip.h must declare the whole ABI"
    # the masked form takes gdr_sim_topk_prefilter's arguments with `flags` in front of the workspace
    base = _ffi.SIGNATURES["gdr_sim_topk_prefilter"][1]
    assert _ffi.PREFILTER_MASK_SIGNATURES["gdr_sim_topk_prefilter_masked"][1] == base[:12] + [C.c_int] + base[12:]


@pytest.mark.parametrize("B,N,d,k", SIZES)
def test_size_is_the_bitmaps_plus_the_unmasked_size(B, N, d, k):
    l = _ffi.lib()
    plain = l.gdr_sim_topk_prefilter_workspace_bytes(B, N, d, k)
    M = gpu.mask_bytes(N)
    assert M == (4 * ((N + 31) // 32) + 255) // 256 * 256 and plain > 0
    assert l.gdr_sim_topk_prefilter_masked_workspace_bytes(B, N, d, k, LIVE) == M + plain
    assert l.gdr_sim_topk_prefilter_masked_workspace_bytes(B, N, d, k, QM) == B * M + plain
    for bad in gpu.REFUSED_FLAGS:
        assert l.gdr_sim_topk_prefilter_masked_workspace_bytes(B, N, d, k, bad) == 0, bad
    for flag in (LIVE, QM):
        assert l.gdr_sim_topk_prefilter_masked_workspace_bytes(0, N, d, k, flag) == 0
        assert l.gdr_sim_topk_prefilter_masked_workspace_bytes(B, 0, d, k, flag) == 0
        assert l.gdr_sim_topk_prefilter_masked_workspace_bytes(B, N, d, 0, flag) == 0


@pytest.mark.parametrize("B,N,d", [(512, 320_000, 768), (40, 20_000, 64), (4, 20_011, 256), (8, 70_001, 128), (4, 1000, 64)])
def test_size_does_not_shrink_as_k_grows(B, N, d):
    """Every k in [1, min(1024, N)]: a buffer sized for a caller's deepest list serves its shallower ones.  One call's own layout is
    not monotone (it dips by up to 2.8 % where a larger k lowers the sample stride by one); the size function answers the largest."""
    l = _ffi.lib()
    for flag in (LIVE, QM):
        sizes = [l.gdr_sim_topk_prefilter_masked_workspace_bytes(B, N, d, k, flag) for k in range(1, min(1024, N) + 1)]
        drops = [k + 1 for k, (a, b) in enumerate(zip(sizes, sizes[1:]), 1) if b < a]
        assert not drops, f"the size shrinks at k = {drops[:8]}"
    own = [gpu.prefilter_plan(B, N, d, k).total for k in range(1, min(1024, N) + 1)]
    assert N <= 16384 or any(b < a for a, b in zip(own, own[1:])), "the restated layout is expected to dip at these shapes"


@pytest.mark.parametrize("B,N,d,k", SIZES[:6])
def test_the_restated_plan_is_the_library_s(B, N, d, k):
    """size = max(largest own layout of any k' <= k, the plain call's size + the bf16 queries + the bands): the restatement of
    make_plan / prefilter_survivor_factor in tests/test_gpu_prefilter_mask.py reproduces the library's answer to the byte."""
    l = _ffi.lib()
    own = max(gpu.prefilter_plan(B, N, d, kk).total for kk in range(1, k + 1))
    plain = l.gdr_sim_topk_workspace_bytes(B, N, d, k, 0) + gpu._up(B * d * 2) + gpu._up(B * 4)
    assert l.gdr_sim_topk_prefilter_workspace_bytes(B, N, d, k) == max(own, plain)
    assert gpu.make_plan(B, N, k).total <= l.gdr_sim_topk_workspace_bytes(B, N, d, k, 0)
    assert gpu.prefilter_plan(B, N, d, k).stride == {(4, 1000, 64, 10): 1, (40, 20_000, 64, 100): 13, (512, 320_000, 768, 100): 55,   # 2500 tiles // 45
                                                     (8, 70_001, 128, 10): 78}.get((B, N, d, k), 39)


def test_refusals_come_before_any_launch():
    """The pointers are never dereferenced: a refused flag combination is GDR_EINVAL whatever the workspace, a workspace one byte short
    GDR_ENOSPC with both sizes in the message, and the unmasked limits (d, k, dnorm_max, alignment) hold for the masked call."""
    l = _ffi.lib()
    p, ws = C.c_void_p(256), C.c_void_p(4096)
    B, N, d, k = 8, 70_001, 128, 10
    call = lambda flags, nbytes, d=d, k=k, norm=1.0, ws=ws: l.gdr_sim_topk_prefilter_masked(p, B, p, p, norm, N, d, k, 0, p, p, None, flags, ws, nbytes, None)   # noqa: E731
    n0 = l.gdr_launch_count()
    for bad in gpu.REFUSED_FLAGS:
        assert call(bad, 1 << 40) == _ffi.GDR_EINVAL, bad
        assert b"exactly GDR_SIM_LIVE_MASK" in l.gdr_last_error()
    for flag in (LIVE, QM):
        need = l.gdr_sim_topk_prefilter_masked_workspace_bytes(B, N, d, k, flag)
        for nbytes in (need - 1, l.gdr_sim_topk_prefilter_workspace_bytes(B, N, d, k)):
            assert call(flag, nbytes) == _ffi.GDR_ENOSPC
            msg = l.gdr_last_error()
            assert str(need).encode() in msg and str(nbytes).encode() in msg, msg
        assert call(flag, need, d=132) == _ffi.GDR_EINVAL and b"d % 8" in l.gdr_last_error()
        assert call(flag, need, d=1032) == _ffi.GDR_EINVAL
        assert call(flag, 1 << 40, k=1025) == _ffi.GDR_EINVAL and b"1024" in l.gdr_last_error()
        assert call(flag, need, norm=0.0) == _ffi.GDR_EINVAL and b"dnorm_max" in l.gdr_last_error()
        assert call(flag, need, ws=C.c_void_p(4096 + 128)) == _ffi.GDR_EINVAL and b"256-byte aligned" in l.gdr_last_error()
        assert l.gdr_sim_topk_prefilter_masked(p, 0, p, p, 1.0, N, d, k, 0, p, p, None, flag, ws, 0, None) == 0   # an empty batch
    assert l.gdr_launch_count() == n0
    # the row-wise upkeep
    up = l.gdr_prefilter_update_rows
    assert up(p, p, 64, None, 0, None, None) == 0                               # n_rows == 0: a no-op
    assert up(p, p, 60, p, 4, p, None) == _ffi.GDR_EINVAL and b"d % 8" in l.gdr_last_error()
    assert up(p, p, 64, p, -1, p, None) == _ffi.GDR_EINVAL
    assert up(p, p, 64, None, 4, p, None) == _ffi.GDR_EINVAL and b"null" in l.gdr_last_error()
    assert up(p, p, 64, p, 4, None, None) == _ffi.GDR_EINVAL
    assert up(C.c_void_p(264), p, 64, p, 4, p, None) == _ffi.GDR_EINVAL and b"aligned" in l.gdr_last_error()
    assert l.gdr_launch_count() == n0


def test_header_states_the_contract():
    text = open(os.path.join(REPO, "include", "gdr_hip_prefilter_mask.h")).read()
    flat = " ".join(text.replace("*", " ").split())
    for phrase in ("exactly GDR_SIM_LIVE_MASK", "ANY upper bound", "never breaks exactness", "only reads", "GDR_ENOSPC before any launch",
                   "NOT zeroed", "no host synchronisation"):
        assert phrase in flat, phrase
    assert "stays UNMASKED" in open(os.path.join(REPO, "include", "gdr_hip.h")).read()   # the unmasked entry point is what it was


# ------------------------------------------------------------------------------------------------------- routing, with stubs
def test_prefilter_route_predicate():
    ok = dict(B=40, d=768, k=100, flags=0, dnorm_max=1.5)
    r = lambda masked, masks, **kw: ops.prefilter_route(*[{**ok, **kw}[n] for n in ("B", "d", "k", "flags", "dnorm_max")], masked, masks)   # noqa: E731
    assert r(False, False) and r(False, True), "the unmasked call takes the pre-filter whatever the flag"
    assert not r(True, False), "the default object keeps masked calls on the plain fp32 path"
    assert r(True, True)
    for masked, masks in ((False, False), (True, True)):
        assert r(masked, masks, k=ops.PREFILTER_MAX_K) and not r(masked, masks, k=ops.PREFILTER_MAX_K + 1)
        assert r(masked, masks, d=1024) and not r(masked, masks, d=1032) and not r(masked, masks, d=764)
        assert not r(masked, masks, flags=_ffi.SIM_EXHAUSTIVE) and r(masked, masks, flags=_ffi.SIM_NO_STREAM)
        assert not r(masked, masks, dnorm_max=0.0) and not r(masked, masks, dnorm_max=float("nan"))
        assert r(masked, masks, B=1)


class _StubCorpus(ops.PrefilteredCorpus):
    """A PrefilteredCorpus that never touches a device: what ops.sim_topk reads before it routes."""

    def __init__(self, N, d, masks, dnorm_max=1.0):
        self.masks, self.dnorm_max = masks, dnorm_max
        self._bind(torch.zeros((N, d)))
        self._D16_buf = torch.zeros((N, d), dtype=torch.bfloat16)


@pytest.mark.parametrize("masks", [False, True])
def test_sim_topk_routes_by_the_flag_of_the_corpus(monkeypatch, masks):
    """ops.sim_topk with its three device entry points stubbed: which one a call reaches, and with which mask arguments."""
    seen = []
    out = lambda Q, k: (torch.zeros((Q.shape[0], k)), torch.zeros((Q.shape[0], k), dtype=torch.int32), torch.zeros(Q.shape[0], dtype=torch.int32))   # noqa: E731
    monkeypatch.setattr(ops, "_need_cuda", lambda *t: None)
    monkeypatch.setattr(ops, "_sim_topk_raw", lambda Q, D, k, off, ws, flags, live=None, allowed=None: seen.append(("raw", flags, live, allowed)) or out(Q, k))
    monkeypatch.setattr(ops, "_sim_topk_prefilter_raw", lambda Q, P, k, off, ws, live=None, allowed=None: seen.append(("pre", 0, live, allowed)) or out(Q, k))
    monkeypatch.setattr(_ffi, "check_device_fault", lambda what: None)
    N, d, B, k = 4096, 64, 4, 10
    P = _StubCorpus(N, d, masks)
    Q = torch.zeros((B, d))
    L = ops.LiveRows.from_bool(torch.ones(N, dtype=torch.bool))
    R = ops.QueryRows.from_bool(torch.ones((B, N), dtype=torch.bool))
    route = "pre" if masks else "raw"
    ops.sim_topk(Q, P, k)
    assert seen[-1] == ("pre", 0, None, None)
    ops.sim_topk(Q, P, k, live=L)
    assert seen[-1][0] == route and seen[-1][2] is L and seen[-1][3] is None
    ops.sim_topk(Q, P, k, allowed=R)
    assert seen[-1][0] == route and seen[-1][2] is None and seen[-1][3] is R
    ops.sim_topk(Q, P, k, live=L, allowed=R)
    assert seen[-1][0] == route and seen[-1][2] is L and seen[-1][3] is R
    for kw in (dict(k=ops.PREFILTER_MAX_K + 1), dict(flags=_ffi.SIM_EXHAUSTIVE)):
        ops.sim_topk(Q, P, kw.get("k", k), live=L, flags=kw.get("flags", 0))
        assert seen[-1][0] == "raw" and seen[-1][2] is L
    assert len(seen) == 6
    # a forced gather capacity is the gather mode's whatever the corpus; "auto" keeps narrow queries there and sends the rest on
    ops.sim_topk(Q, P, k, allowed=R, gather=4096)
    assert seen[-1][0] == "raw" and seen[-1][1] & _ffi.SIM_ROW_GATHER
    mixed = torch.ones((B, N), dtype=torch.bool)
    mixed[1, 100:] = False
    monkeypatch.setattr(ops, "GATHER_MAX_ROWS", 1000)
    n = len(seen)
    ops.sim_topk(Q, P, k, allowed=ops.QueryRows.from_bool(mixed), gather="auto")
    assert [(c[0], bool(c[1] & _ffi.SIM_ROW_GATHER), c[3].B) for c in seen[n:]] == [("raw", True, 1), (route, False, 3)]


def test_restated_occupancy_counts_what_the_lists_hold():
    """occupancy() on a hand-made case: 4 sample-tile rows and 6 others, k = 2."""
    S = np.array([[9.0, 8.0, 7.0, 1.0] + [0.0] * 124 + [8.5, 7.5, 6.0, 5.0, 7.2, 7.1] + [0.0] * 20_000])
    N = S.shape[1]
    p = gpu.prefilter_plan(1, N, 64, 2)
    assert p.stride > 1 and gpu.in_sample_tile(N, p.stride)[:128].all() and not gpu.in_sample_tile(N, p.stride)[128:256].any()
    a = np.ones((1, N), bool)
    Q = np.full((1, 64), 1e-3)                                                # eps2 ~ 1e-4: far below the score gaps
    longest, cap, fullest, cap2, no_thr = gpu.occupancy(S, a, Q, 1.0, 64, 2)
    assert (longest - p.n_slots, cap, fullest, cap2, no_thr) == (1, p.cap, 2, 1024, [])   # 8.5 alone reaches the threshold 8.0; band {9, 8.5}
    a[0, :2] = False                                                          # the two best sample rows die: threshold 1.0, band {8.5, 7.5}
    longest, _, fullest, _, _ = gpu.occupancy(S, a, Q, 1.0, 64, 2)
    assert (longest - p.n_slots, fullest) == (6, 2)
    a[0, 2] = False                                                           # one allowed sample row with a score... 125 zeros remain: k = 2 holds
    assert gpu.occupancy(S, a, Q, 1.0, 64, 2)[4] == []
    a[0, gpu.in_sample_tile(N, p.stride)] = False
    a[0, 3] = True
    assert gpu.occupancy(S, a, Q, 1.0, 64, 2)[4] == [0]
