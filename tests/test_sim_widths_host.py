"""The inputs of the width sweep (tests/sim_widths.py), checked from the inputs alone: the integer scores are exact in fp32 and in
bf16, the expected lists are np.lexsort((ids, -scores))[:k], a planted tie sits inside every list shape, and no candidate list of the
two-pass shapes can overflow — so tests/test_gpu_sim_widths.py may compare with torch.equal and demand status 0.  Needs no GPU."""
import numpy as np
import pytest
import torch

import sim_widths as sw

ALL_WIDTHS = sorted(set(sw.widths("fp32")) | set(sw.widths("bf16")) | set(sw.PREFILTER))


def test_the_plan_rule_gives_the_documented_figures():
    assert sw.plan(sw.N_BIG, sw.K_BIG) == (39, 640, 6016)
    assert sw.plan(320_000, 1024)[::2] == (17, 92_288) and sw.plan(320_000, 8192)[::2] == (6, 253_952)     # include/gdr_hip.h
    assert sw.plan(140_001, 8192)[1:] == (35_072, 169_984)                                                 # tests/test_gpu_sim_deep_k.py
    for N, k in sw.ONE_PASS:
        assert sw.plan(N, k)[0] == 1
    tiles = -(-sw.N_BIG // sw.TILE)
    assert tiles == 157 and sw.N_BIG - 156 * sw.TILE == 33
    for k in (1, 10, 100):                                     # the 33-row tile is sampled at every depth that runs
        stride = sw.plan(sw.N_BIG, k)[0]
        assert stride > 1 and 156 % stride == 0, (k, stride)
        assert sw.sample_rows(sw.N_BIG, stride).size == (156 // stride) * 128 + 33


def test_the_library_lays_out_at_least_the_plan():
    """gdr_sim_topk_workspace_bytes answers with the largest plan up to k: never less than 8 bytes per entry of plan()'s list"""
    from gdr_amd import _ffi
    l = _ffi.lib()
    for k in (1, 10, 100):
        cap = sw.plan(sw.N_BIG, k)[2]
        for B in (7, 129):
            got = l.gdr_sim_topk_workspace_bytes(B, sw.N_BIG, 768, k, 0)
            assert got >= B * cap * 8, (k, B, got, cap)
    assert 0 <= l.gdr_sim_topk_workspace_bytes(129, sw.N_BIG, 768, 1, 0) - 129 * sw.plan(sw.N_BIG, 1)[2] * 8 <= 129 * 132 + 4 * 256


def test_every_width_of_the_contract_is_listed_once():
    f32, b16 = sw.widths("fp32"), sw.widths("bf16")
    assert len(set(f32)) == len(f32) and len(set(b16)) == len(b16)
    assert all(d % 4 == 0 for d in f32) and all(d % 8 == 0 for d in b16) and all(d % 8 == 0 and d <= 1024 for d in sw.PREFILTER)
    assert [d for d in f32 if sw.stream_eligible("fp32", d)] == list(sw.F32_STREAM)
    assert [d for d in b16 if sw.stream_eligible("bf16", d)] == list(sw.BF16_STREAM)
    assert all(d % 32 for d in sw.F32_TILED if d not in (32, 64)) and all(d % 64 for d in sw.BF16_GENERIC)
    assert all(d % 64 == 0 and d % 256 for d in sw.BF16_GLDS)
    assert sorted(d // 32 for d in sw.F32_STREAM) == [4, 8, 12, 16, 20, 24, 28, 32]          # groups of the fp32 ring
    assert sorted(d // 64 for d in sw.BF16_STREAM) == [4, 8, 12, 16, 20, 24, 28, 32]         # groups of the bf16 ring
    assert sum(1 for d in sw.PREFILTER if d % 256) == 6                                 # the rescoring's guard splits a piece
    assert [b for b, _ in sw.batches("fp32", 36)] == [7, 129]
    assert [b for b, ns in sw.batches("fp32", 896) if not ns] == [1, 7, 32, 33, 128, 129]
    assert [b for b, ns in sw.batches("bf16", 2048) if ns] == [1, 7, 32]


@pytest.mark.parametrize("d", ALL_WIDTHS)
def test_integer_inputs_are_exact_and_tied_and_cannot_overflow(d):
    R = sw.radius(d)
    assert R == min(127, int(np.floor(np.sqrt(2 ** 23 / d)))) and d * R * R < 2 ** 24
    Q, D = sw.ints(d)
    assert Q.shape == (sw.B_MAX, d) and D.shape == (sw.N_BIG, d) and Q.dtype == D.dtype == np.float32
    for x in (Q, D):
        assert np.array_equal(x, np.rint(x)) and np.abs(x).max() <= R
        t = torch.from_numpy(x)
        assert torch.equal(t.bfloat16().float(), t)
    s = sw.int_scores(d)
    assert np.abs(s).max() <= d * R * R
    rows = np.r_[0:130, 10_000:10_064, sw.N_BIG - 64:sw.N_BIG]         # the integer product itself, where numpy has no BLAS for it
    assert np.array_equal(s[:, rows], Q.astype(np.int64) @ D[rows].astype(np.int64).T)
    f = Q @ D.T
    assert f.dtype == np.float32 and np.array_equal(f.astype(np.int64), s) and np.array_equal(f, s.astype(np.float32))
    ids = np.arange(sw.N_BIG)
    depths = [(sw.N_BIG, k) for k in (1, 100)] if any(d in w for w in sw.DEEP_WIDTHS.values()) or d in sw.PREFILTER_K100 else []
    for N, k in list(sw.SHAPES) + depths:
        ev, ei = sw.expected(d, N, k)
        assert ev.shape == ei.shape == (sw.B_MAX, k) and ev.dtype == torch.float32 and ei.dtype == torch.int32
        for q in (0, 1, 7, 128):                                       # the expected list IS the lexsort
            order = np.lexsort((ids[:N], -s[q, :N]))[:k]
            assert np.array_equal(ei[q].numpy(), order) and np.array_equal(ev[q].numpy(), s[q, order].astype(np.float32)), (N, k, q)
        v = ev.numpy()
        cut_all = (s[:, :N] == v[:, -1:].astype(np.int64)).sum(1)
        cut_in = (v == v[:, -1:]).sum(1)
        tied = (v[:, 1:] == v[:, :-1]).any(1) | (cut_in < cut_all)     # a tie inside the list, or the cut splits a tie group
        assert tied[0], (N, k, "query 0 has no tie: the lower-id rule is not exercised")
        if k > 1:
            assert (v[0, 1:] == v[0, :-1]).any(), (N, k)
        else:
            assert cut_all[0] > 1 and ei[0, 0] == np.flatnonzero(s[0, :N] == s[0, :N].max())[0]
    for N, k in [(sw.N_BIG, sw.K_BIG)] + depths:                       # two-pass shapes: the reference alone shows that no list overflows
        stride, slots, cap = sw.plan(N, k)
        assert stride > 1
        n, thr = sw.survivors(s, N, k)
        print(f"d={d} k={k}: stride {stride}, {slots} sample slots, capacity {cap}; rows at or above the sample's k-th best: max {n.max()}")
        assert n.max() < cap // 2 and slots + n.max() <= cap, (k, int(n.max()), cap)
        if d in sw.PREFILTER and (k == sw.K_BIG or (k == 100 and d in sw.PREFILTER_K100)):
            # the pre-filter keeps s~ >= L - 2 eps_q in a list never smaller than the plain one, and rescores the band
            # s~ >= t_k - 2 eps_q, at most max(1024, 4k) rows; the bf16-operand scores s~ are these integers
            B = max(sw.PREFILTER_B)
            eps2 = sw.prefilter_eps2(Q[:B], D)
            kept = (s[:B] >= (thr[:B] - eps2)[:, None]).sum(1)
            tk = np.sort(s[:B], axis=1)[:, -k]
            band = (s[:B] >= (tk - eps2)[:, None]).sum(1)
            print(f"d={d} k={k} pre-filter: kept max {kept.max()} of {cap}, band max {band.max()} of 1024")
            assert slots + kept.max() <= cap and band.max() <= 1024, (k, int(kept.max()), int(band.max()))


@pytest.mark.parametrize("kind,d", [(kind, d) for kind, ws in sw.FLOAT_WIDTHS.items() for d in ws])
def test_float_inputs_put_half_of_the_norm_into_the_end_pieces(kind, d):
    Q, D = sw.floats(kind, d)
    piece = 8 if kind == "bf16" else 4
    for x in (Q, D):
        x = x.astype(np.float64)
        assert np.allclose((x ** 2).sum(1), 1.0, atol=1e-5)
        ends = (x[:, :piece] ** 2).sum(1) + (x[:, -piece:] ** 2).sum(1)
        assert np.allclose(ends, 0.5, atol=1e-5)
    Q64, D64, s = sw.float_reference(kind, d)
    tol, band = sw.float_tolerance(kind, d, Q64, D64)
    assert tol == max(1e-5 if kind == "bf16" else 1e-4, band) and band < 3e-4
    # what one end piece contributes to a score dwarfs the tolerance: its rms over (query, row) is about 0.25 / sqrt(piece)
    last = Q64[:, -piece:] @ D64[:, -piece:].T
    assert np.sqrt((last ** 2).mean()) > 0.05 > 100 * tol
    n, _ = sw.survivors(s, sw.FLOAT_N, sw.FLOAT_K)
    assert n.max() < sw.plan(sw.FLOAT_N, sw.FLOAT_K)[2] // 2


@pytest.mark.parametrize("d", sw.RERANK_WIDTHS)
def test_rerank_case_is_well_formed(d):
    c = sw.rerank_case(d)
    assert c["sizes"].min() == 5 and c["sizes"].max() == 40 and c["offsets"][-1] == c["ids"].size == c["sizes"].sum()
    for b, m in enumerate(c["mem"]):
        assert len(set(m)) == len(m) == c["sizes"][b].sum() >= c["k"]
    s = c["Q"].astype(np.float64) @ c["D"].astype(np.float64).T
    assert np.abs(s).max() < 0.95
