"""The argument range of the corpus-wide top-k past k = 1024, checked on the host: gdr_sim_topk, gdr_sim_topk_bf16, gdr_topk_merge,
gdr_topk_pack and gdr_topk_merge_packed take 1 <= k <= 8192 (one LDS sort, select.h SEL_SORT_MAX); gdr_sim_topk_prefilter stays at
1024 with its refusal text.  Every call below is refused by an argument or size check BEFORE anything is launched: the pointers are
dummies that are never dereferenced (as in tests/test_abi_memory_host.py).  Needs no GPU."""
import ctypes as C

from gdr_amd import _ffi, ops

P, WS = C.c_void_p(256), C.c_void_p(4096)
N, B, D_, G = 70_001, 8, 128, 3
BIG = 1 << 40


def _calls(l):
    return (
        ("gdr_sim_topk", lambda k, nbytes=BIG: l.gdr_sim_topk(P, B, P, N, D_, k, 0, P, P, None, 0, WS, nbytes, None)),
        ("gdr_sim_topk_bf16", lambda k, nbytes=BIG: l.gdr_sim_topk_bf16(P, B, P, N, D_, k, 0, P, P, None, 0, WS, nbytes, None)),
        ("gdr_topk_merge", lambda k: l.gdr_topk_merge(P, P, G, B, k, P, P, None)),
        ("gdr_topk_pack", lambda k: l.gdr_topk_pack(P, P, None, B, k, P, None)),
        ("gdr_topk_merge_packed", lambda k: l.gdr_topk_merge_packed(P, G, B, k, P, P, None, None)),
    )


def test_k_8193_is_refused_with_the_new_limit_in_the_message():
    l = _ffi.lib()
    for name, call in _calls(l):
        assert call(8193) == _ffi.GDR_EINVAL, name
        assert b"8192" in l.gdr_last_error(), (name, l.gdr_last_error())
        assert call(0) == _ffi.GDR_EINVAL, name
    assert l.gdr_sim_topk(P, B, P, 4000, D_, 4001, 0, P, P, None, 0, WS, BIG, None) == _ffi.GDR_EINVAL      # k <= N still holds
    assert b"k=4001" in l.gdr_last_error()


def test_the_prefilter_still_stops_at_1024():
    l = _ffi.lib()
    assert l.gdr_sim_topk_prefilter(P, B, P, P, 1.0, N, D_, 1025, 0, P, P, None, WS, BIG, None) == _ffi.GDR_EINVAL
    msg = l.gdr_last_error()
    assert msg == b"sim_topk_prefilter: k=1025 must be in [1, min(1024, N)]", msg


def test_k_8192_passes_the_argument_check_and_stops_at_the_size_check():
    """A 256-byte workspace: GDR_ENOSPC, i.e. k = 8192 (and 1025) got past the argument checks and the size check caught the call
    before any launch."""
    l = _ffi.lib()
    for name, call in _calls(l)[:2]:
        for k in (1025, 8192):
            assert call(k, 256) == _ffi.GDR_ENOSPC, (name, k, l.gdr_last_error())
            assert b"workspace 256 < required" in l.gdr_last_error()


def test_workspace_bytes_is_monotone_in_k():
    """gdr_sim_topk_workspace_bytes non-decreasing in k from 1 to 8192, at the two batch sizes whose sizes the header documents and at
    the shape of the deep-k GPU tests: a buffer sized for a caller's deepest list serves its shallower ones.  The plan of ONE call is
    not monotone (each time a larger k lowers the sample stride by one the sample block grows by a step while the survivor term
    4 k N / n_sample shrinks: 59 dips of 1 - 2 % in [1, 8192] at N = 320 000, the first at k = 20 -> 21, 5 371 136 -> 5 289 216
    bytes at 40 queries), so the entry point answers with the largest plan up to k."""
    l = _ffi.lib()
    for b, n in ((40, 320_000), (512, 320_000), (3, 70_001)):
        sizes = [l.gdr_sim_topk_workspace_bytes(b, n, 768, k, 0) for k in range(1, 8193)]
        dips = [(k + 2, x, y) for k, (x, y) in enumerate(zip(sizes, sizes[1:])) if y < x]
        print(f"B={b} N={n}: {len(dips)} dips, first {dips[:2]}")
        assert sizes[0] > 0 and not dips, (b, n, len(dips), dips[:3])


def test_workspace_bytes_gives_the_documented_sizes():
    """include/gdr_hip.h, DESIGN.md §4: N = 320 000, k = 8192 -> stride 6, a list of 253 952 entries of 8 bytes per query; beside it
    128 bytes of counters per query, the thresholds, the sliced tails' partial lists at B <= 32, and alignment."""
    l = _ffi.lib()
    for b, mib in ((40, 77.5), (512, 992.1)):
        got = l.gdr_sim_topk_workspace_bytes(b, 320_000, 768, 8192, 0)
        assert 0 <= got - b * 253_952 * 8 <= b * (128 + 4) + 4 * 256, (b, got)
        assert abs(got / 2 ** 20 - mib) < 0.05, (b, got)
    assert abs(l.gdr_sim_topk_workspace_bytes(512, 320_000, 768, 1024, 0) / 2 ** 20 - 360.6) < 0.05      # k = 1024: as before
    assert l.gdr_sim_topk_workspace_bytes(8, 70_001, 768, 8192, 0) > l.gdr_sim_topk_workspace_bytes(8, 70_001, 768, 1024, 0) > 0


def test_the_ops_constants_are_the_refusals():
    """One past each constant is GDR_EINVAL; the constant itself passes the argument check (shown where a size check stands behind
    it to stop the call: the merges and the pack have none, their deep k runs in tests/test_gpu_sim_deep_k.py)."""
    l = _ffi.lib()
    assert ops.SIM_TOPK_MAX_K == 8192 and ops.PREFILTER_MAX_K == 1024
    calls = _calls(l)
    for name, call in calls:
        assert call(ops.SIM_TOPK_MAX_K + 1) == _ffi.GDR_EINVAL, name
    for name, call in calls[:2]:
        assert call(ops.SIM_TOPK_MAX_K, 256) == _ffi.GDR_ENOSPC, name
    assert l.gdr_sim_topk_prefilter(P, B, P, P, 1.0, N, D_, ops.PREFILTER_MAX_K + 1, 0, P, P, None, WS, BIG, None) == _ffi.GDR_EINVAL
    assert l.gdr_sim_topk_prefilter(P, B, P, P, 1.0, N, D_, ops.PREFILTER_MAX_K, 0, P, P, None, WS, 256, None) == _ffi.GDR_ENOSPC
