"""The gather mode of the filtered corpus search, host side: flag values, the workspace sizing and the pre-launch
errors of gdr_sim_topk's GDR_SIM_ROW_GATHER, ops.gather_route and tests/gather_ref.py on hand-written cases.  Needs no GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import gather_ref
import live_ref
from conftest import REPO
from gdr_amd import _ffi, ops
from test_query_mask_host import PLAIN

QM, RG = 8, 16
SHAPES = [(8, 70_001, 10), (512, 320_000, 100), (4, 1000, 10)]


def test_flag_and_field_values():
    assert _ffi.SIM_ROW_GATHER == RG
    assert RG & (_ffi.SIM_EXHAUSTIVE | _ffi.SIM_NO_STREAM | _ffi.SIM_LIVE_MASK | _ffi.SIM_QUERY_MASK) == 0
    assert [_ffi.sim_gather_chunks(c) for c in (0, 1, 2, 3, 256)] == [0, 256, 512, 768, 65536]
    assert _ffi.sim_gather_chunks(256) & 0xFF == 0 and _ffi.sim_gather_chunks(256) < 1 << 17
    text = open(os.path.join(REPO, "include", "gdr_hip.h")).read()
    assert "#define GDR_SIM_ROW_GATHER 16" in text
    assert "#define GDR_SIM_GATHER_CHUNKS(c) ((c) << 8)" in text
    assert "stays UNMASKED" in text


@pytest.mark.parametrize("B,N,k", SHAPES)
def test_workspace_holds_the_bitmaps_and_the_lists_and_grows_with_the_capacity(B, N, k):
    """Fails without the feature: bit 16 and bits 8..16 of flags were ignored, so the size did not move with c."""
    l = _ffi.lib()
    sizes = []
    for c in (1, 2, 3, 256):
        f = QM | RG | _ffi.sim_gather_chunks(c)
        need = l.gdr_sim_topk_workspace_bytes(B, N, 64, k, f)
        assert need >= B * live_ref.mask_bytes(N) + 8 * B * 4096 * c
        assert need == l.gdr_sim_topk_workspace_bytes(B, N, 768, k, f), "the size depends on d"
        assert need == l.gdr_sim_topk_workspace_bytes(B, N, 64, k, f | _ffi.SIM_NO_STREAM)
        # the layout behind the bitmaps does not depend on N
        other = l.gdr_sim_topk_workspace_bytes(B, 2 * N, 64, k, f)
        assert need - B * live_ref.mask_bytes(N) == other - B * live_ref.mask_bytes(2 * N)
        sizes.append(need)
    assert sizes == sorted(set(sizes)), "strictly increasing in c"
    assert l.gdr_sim_topk_workspace_bytes(B, N, 64, k, QM | RG) == sizes[1], "a chunk field of 0 reads as 2"
    for c in (1, 2, 3, 256):                                                  # non-decreasing in k
        f = QM | RG | _ffi.sim_gather_chunks(c)
        by_k = [l.gdr_sim_topk_workspace_bytes(B, N, 64, kk, f) for kk in (1, 10, 100, 1000, 1024) if kk <= N]
        assert by_k == sorted(by_k)


@pytest.mark.parametrize("B,N,k", list(PLAIN))
def test_sizes_without_the_new_bits_are_what_they_were(B, N, k):
    l = _ffi.lib()
    for d in (64, 768):
        assert l.gdr_sim_topk_workspace_bytes(B, N, d, k, 0) == PLAIN[(B, N, k)][0]
        assert l.gdr_sim_topk_workspace_bytes(B, N, d, k, _ffi.SIM_EXHAUSTIVE) == PLAIN[(B, N, k)][1]
        assert l.gdr_sim_topk_workspace_bytes(B, N, d, k, QM) == PLAIN[(B, N, k)][0] + B * live_ref.mask_bytes(N)
        assert l.gdr_sim_topk_workspace_bytes(B, N, d, k, _ffi.SIM_LIVE_MASK) == PLAIN[(B, N, k)][0] + live_ref.mask_bytes(N)


EINVAL_CASES = [
    # (flags, k, words the message must hold)
    (RG, 10, [b"GDR_SIM_ROW_GATHER", b"GDR_SIM_QUERY_MASK"]),                                    # without the query mask
    (RG | _ffi.SIM_LIVE_MASK, 10, [b"GDR_SIM_ROW_GATHER", b"GDR_SIM_LIVE_MASK"]),                # with the live mask
    (RG | QM | _ffi.SIM_LIVE_MASK, 10, [b"GDR_SIM_LIVE_MASK"]),
    (RG | QM | _ffi.SIM_EXHAUSTIVE, 10, [b"GDR_SIM_ROW_GATHER", b"GDR_SIM_EXHAUSTIVE"]),         # with the exhaustive plan
    (RG | QM | _ffi.sim_gather_chunks(257), 10, [b"GDR_SIM_ROW_GATHER", b"257"]),                # a chunk field above 256
    (RG | QM | _ffi.sim_gather_chunks(511), 10, [b"GDR_SIM_ROW_GATHER", b"511"]),
    (QM | _ffi.sim_gather_chunks(1), 10, [b"GDR_SIM_ROW_GATHER", b"GDR_SIM_GATHER_CHUNKS"]),     # a chunk field without the flag
    (_ffi.sim_gather_chunks(3), 10, [b"GDR_SIM_ROW_GATHER", b"GDR_SIM_GATHER_CHUNKS"]),
    (RG | QM | _ffi.sim_gather_chunks(3), 1025, [b"GDR_SIM_ROW_GATHER", b"1025", b"1024"]),      # k > 1024 with c > 2
]


@pytest.mark.parametrize("flags,k,words", EINVAL_CASES)
def test_refused_before_any_launch(flags, k, words):
    """Null-ish pointers: nothing is dereferenced.  The size asked for such a call is 0."""
    l = _ffi.lib()
    p, ws = C.c_void_p(256), C.c_void_p(4096)
    for fn in (l.gdr_sim_topk, l.gdr_sim_topk_bf16):
        assert fn(p, 8, p, 70_001, 64, k, 0, p, p, None, flags, ws, 1 << 40, None) == _ffi.GDR_EINVAL, hex(flags)
        msg = l.gdr_last_error()
        assert all(w in msg for w in words), msg
    assert l.gdr_sim_topk_workspace_bytes(8, 70_001, 64, k, flags) == 0


def test_accepted_combinations_reach_the_size_check():
    """k > 1024 at c <= 2, k = 1024 at c = 256, GDR_SIM_NO_STREAM: valid calls, stopped here by a workspace one byte short."""
    l = _ffi.lib()
    p, ws = C.c_void_p(256), C.c_void_p(4096)
    for fn in (l.gdr_sim_topk, l.gdr_sim_topk_bf16):
        for c, k, more in ((0, 8192, 0), (1, 2000, 0), (2, 8192, _ffi.SIM_NO_STREAM), (3, 1024, 0), (256, 1024, 0), (256, 1, _ffi.SIM_NO_STREAM)):
            for (B, N) in ((8, 70_001), (512, 320_000)):
                flags = QM | RG | _ffi.sim_gather_chunks(c) | more
                need = l.gdr_sim_topk_workspace_bytes(B, N, 64, k, flags)
                assert need > 0
                assert fn(p, B, p, N, 64, k, 0, p, p, None, flags, ws, need - 1, None) == _ffi.GDR_ENOSPC, (c, k, B, N)
                msg = l.gdr_last_error()
                assert str(need).encode() in msg and str(need - 1).encode() in msg, msg


def test_gather_route_on_hand_written_counts():
    M = ops.GATHER_MAX_ROWS
    assert M % 4096 == 0 and M >= 4096
    assert ops.gather_route([], 10, M) == ([], 0)
    assert ops.gather_route([0], 10, M) == ([0], 1)
    assert ops.gather_route([1], 10, M) == ([0], 1)
    assert ops.gather_route([M], 10, M) == ([0], M // 4096)
    assert ops.gather_route([M + 1], 10, M) == ([], 0)
    assert ops.gather_route([M + 1, 0, 4096, 4097, 320_000, 7], 10, M) == ([1, 2, 3, 5], 2)
    assert ops.gather_route([5000, 100_000, 12_289], 100, 16_384) == ([0, 2], 4)
    # k = 2000 with 9 000 rows: the chunked regime stops at k = 1024, the query stays on the dense route
    assert ops.gather_route([9000], 2000, 16_384) == ([], 0)
    assert ops.gather_route([9000, 8192], 2000, 16_384) == ([1], 2)
    assert ops.gather_route([9000], 1024, 16_384) == ([0], 3)
    assert ops.gather_route([2 ** 20, 2 ** 20 + 1], 10, 2 ** 30) == ([0], 256)
    assert [ops.gather_chunks(r) for r in (1, 4096, 4097, 8192, 8193)] == [1, 1, 2, 2, 3]


def test_gather_ref_against_hand_cases():
    assert gather_ref.cap_of(0) == 8192 and gather_ref.cap_of(1) == 4096 and gather_ref.cap_of(256) == 2 ** 20
    a = np.zeros((4, 70), bool)
    a[0, [3, 31, 32, 69]] = True
    a[1] = True
    a[3, 5] = True
    w = live_ref.pack(a[0]).copy()
    w[-1] |= np.int32(-1) << np.int32(70 % 32)                               # garbage past N is ignored
    rows, count = gather_ref.rows_of(w, 70, 3)
    assert rows.tolist() == [3, 31, 32] and count == 4
    assert gather_ref.rows_of(live_ref.pack(a[2]), 70, 3) [0].size == 0
    S = np.tile(np.arange(70, dtype=np.float64), (4, 1))                      # the score of a row is its number ...
    S[1, 2] = S[1, 0] = 9.0                                                   # ... but rows 0, 2 and 9 of query 1 tie
    v, i, st = gather_ref.topk(S, a, 3, 5, idx_offset=100)
    assert st.tolist() == [0, 1, 0, 0]
    assert i[0].tolist() == [169, 132, 131] and v[0].tolist() == [69.0, 32.0, 31.0]
    assert i[1].tolist() == [100, 102, 104] and v[1].tolist() == [9.0, 9.0, 4.0]   # the first 5 rows only; the lower id wins the tie
    assert i[2].tolist() == [-1, -1, -1] and np.isneginf(v[2]).all()
    assert i[3].tolist() == [105, -1, -1] and v[3, 0] == 5.0 and np.isneginf(v[3, 1:]).all()
