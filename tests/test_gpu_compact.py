"""Compacting a live corpus on the MI355X (include/gdr_hip_compact.h): gdr_rows_compact_plan, gdr_rows_compact,
gdr_ids_remap and gdr_rowmask_compact against the numpy restatement (tests/compact_ref.py), their memory contract
(tests/abi_guard.py), a captured graph, and GDRRetriever.compact_documents end to end.  Integers and bytes are compared exactly."""
import types

import numpy as np
import pytest
import torch

import compact_ref
import expand_ref
import lifecycle_ref
import live_ref
from abi_guard import guarded, guarded_input, poisoned_workspace
from conftest import order_insensitive_topk_match
from gdr_amd import _ffi, codec, ops, synth
from gdr_amd._ffi import lib, ptr, stream_ptr
from gdr_amd.config import GDRConfig

pytestmark = pytest.mark.gpu

TOL = 1e-4                         # oracle/parity_rules.py, as tests/test_gpu_live_search.py uses it
# csrc/compact.hip: a wave sweeps a chunk of 64 bitmap words (PLAN_CHUNK_ROWS), a tile is PLAN_TILE_WORDS = 128 words (a wave per
# tile), a workgroup holds 4 waves (PLAN_BLOCK_ROWS), and the one-workgroup scan (csrc/scan.h BlockScan) takes PLAN_SCAN_STEP = 1024
# tiles per round
PLAN_CHUNK_ROWS = 64 * 32
PLAN_TILE_ROWS = 128 * 32
PLAN_BLOCK_ROWS = 4 * PLAN_TILE_ROWS
PLAN_SCAN_ROWS = 1024 * PLAN_TILE_ROWS
PLAN_NS = [1, 31, 32, 33, 63, 64, 65, 1000, 20_011] + [c + e for c in (PLAN_CHUNK_ROWS, PLAN_TILE_ROWS, PLAN_BLOCK_ROWS) for e in (-1, 0, 1)]
SCAN_NS = [PLAN_SCAN_ROWS + e for e in (-1, 0, 1)]
ROW_BYTES = [4, 12, 200, 192, 256, 1536, 3072]    # 200 = int64 x 25 (the 4-byte path), 192 = int64 x 24, 1536 = bf16 x 768
SENTINEL = -123456789


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    torch.set_grad_enabled(False)
    return torch.device("cuda:0")


def _masks(N, seed=0, few=False):
    """name -> live bool [N]."""
    rng = np.random.default_rng(N + seed)
    m = {"all live": np.ones(N, bool), "random 50 % dead": rng.random(N) >= 0.5, "alternating": np.arange(N) % 2 == 0}
    if few:
        return m
    m["all dead"] = np.zeros(N, bool)
    for name, dead in (("only row 0 dead", [0]), ("only the last row dead", [N - 1])):
        m[name] = np.ones(N, bool)
        m[name][dead] = False
    m["only row 0 live"] = np.zeros(N, bool)
    m["only row 0 live"][0] = True
    runs = np.ones(N, bool)                                                    # dead runs on word boundaries
    off = np.ones(N, bool)                                                     # and one bit off them, at either end
    for lo, hi in ((32, 96), (128, 160), (N // 2 // 32 * 32, N // 2 // 32 * 32 + 64), (max(N - 64, 0) // 32 * 32, N)):
        runs[lo:hi] = False
        off[lo + 1:max(hi - 1, 0)] = False
        off[max(lo - 1, 0):lo] = False
    m["dead runs on word boundaries"], m["dead runs one bit off word boundaries"] = runs, off
    for pct in (1, 99):
        m[f"random {pct} % dead"] = rng.random(N) >= pct / 100
    return m


def _up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _plan_raw(words_d, N, n_live, dev, tail=8):
    """The C entry point with a workspace of exactly the declared size and sentinels behind both outputs."""
    new_id = torch.full((N + tail,), SENTINEL, dtype=torch.int32, device=dev)
    old_id = torch.full((n_live + tail,), SENTINEL, dtype=torch.int32, device=dev)
    status = torch.full((2,), SENTINEL, dtype=torch.int32, device=dev)
    need = lib().gdr_rows_compact_plan_workspace_bytes(N)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    rc = lib().gdr_rows_compact_plan(ptr(words_d), N, n_live, ptr(new_id), ptr(old_id), ptr(status), ptr(ws), need, stream_ptr())
    assert rc == 0, lib().gdr_last_error().decode()
    return new_id, old_id, status


def _dirty(words, N):
    """The bitmap with every bit past N set in its last word."""
    w = words.copy().view(np.uint32)
    if N % 32:
        w[-1] |= np.uint32((0xFFFFFFFF << (N % 32)) & 0xFFFFFFFF)
    return w.view(np.int32)


# ------------------------------------------------------------------------------------------------------------------- the plan
@pytest.mark.parametrize("N", PLAN_NS + SCAN_NS)
def test_plan_matches_the_restatement(dev, N):
    for name, live in _masks(N, few=N in SCAN_NS).items():
        want_new, want_old = compact_ref.plan(live)
        n_live = int(live.sum())
        words = compact_ref.pack(live)
        for variant, w in (("clean", words), ("bits past N set", _dirty(words, N))):
            new_id, old_id, status = _plan_raw(_up(w, dev), N, n_live, dev)
            what = f"N={N}, {name}, {variant}"
            assert status.tolist() == [0, SENTINEL], what
            assert np.array_equal(new_id[:N].cpu().numpy(), want_new), what
            assert np.array_equal(old_id[:n_live].cpu().numpy(), want_old), what
            assert (new_id[N:] == SENTINEL).all() and (old_id[n_live:] == SENTINEL).all(), what


@pytest.mark.parametrize("N", [1, 65, 1000, PLAN_TILE_ROWS + 1, 20_011])
def test_plan_reports_a_wrong_count_and_stays_inside_its_outputs(dev, N):
    for name, live in _masks(N).items():
        n_live = int(live.sum())
        words_d = _up(compact_ref.pack(live), dev)
        for wrong in (n_live - 1, n_live + 1):
            if not 0 <= wrong <= N:
                continue
            new_id, old_id, status = _plan_raw(words_d, N, wrong, dev)
            what = f"N={N}, {name}, n_live={wrong} for {n_live}"
            assert status.tolist() == [1, SENTINEL], what
            assert (new_id[N:] == SENTINEL).all() and (old_id[wrong:] == SENTINEL).all(), what


# ------------------------------------------------------------------------------------------------------------------- the rows
def _rows_raw(src, dst, N, row_bytes, old_id_d, n_live, chunk_rows, dev, ws=None):
    """src / dst: tensors or raw addresses."""
    addr = lambda t: t if isinstance(t, int) else t.data_ptr()   # noqa: E731
    need = lib().gdr_rows_compact_workspace_bytes(row_bytes, chunk_rows) if addr(src) == addr(dst) else 0
    if ws is None and need:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
    rc = lib().gdr_rows_compact(addr(src), addr(dst), N, row_bytes, ptr(old_id_d) if n_live else None, n_live, chunk_rows, ptr(ws),
                                need, stream_ptr())
    assert rc == 0, lib().gdr_last_error().decode()


@pytest.mark.parametrize("row_bytes", ROW_BYTES)
def test_rows_match_the_restatement_out_of_place_and_in_place(dev, row_bytes):
    """N = 5000 with chunks of 64, 4096, the default and one larger than n_live; N = 300 with chunks of one row.  Dead runs of 64
    and more rows straddle the chunk boundaries in every mask."""
    rng = np.random.default_rng(row_bytes)
    for N, chunks in ((5000, (64, 4096, 0, 10_000)), (300, (1, 64))):
        T = rng.integers(-2 ** 31, 2 ** 31, (N, row_bytes // 4), dtype=np.int64).astype(np.int32)
        Td = _up(T, dev)
        for name, live in _masks(N, seed=row_bytes).items():
            _new, old = compact_ref.plan(live)
            n_live, old_d = old.size, _up(old, dev)
            want = _up(compact_ref.rows_in_place(T, old), dev)
            what = f"row_bytes={row_bytes}, N={N}, {name}"
            out = torch.full((n_live + 3, row_bytes // 4), SENTINEL, dtype=torch.int32, device=dev)
            _rows_raw(Td, out, N, row_bytes, old_d, n_live, 0, dev)
            assert torch.equal(out[:n_live], want[:n_live]) and (out[n_live:] == SENTINEL).all(), what + ", out of place"
            assert torch.equal(Td, _up(T, dev)), what + ": the source of the out-of-place form changed"
            for chunk in chunks:
                t = Td.clone()
                _rows_raw(t, t, N, row_bytes, old_d, n_live, chunk, dev)
                assert torch.equal(t, want), what + f", in place, chunk_rows={chunk}"   # rows >= n_live hold what they held


@pytest.mark.parametrize("row_bytes", [192, 256, 3072])
def test_rows_from_a_base_offset_by_4_bytes_take_the_4_byte_path_with_the_same_bytes(dev, row_bytes):
    N = 1000
    rng = np.random.default_rng(row_bytes + 1)
    T = rng.integers(-2 ** 31, 2 ** 31, (N, row_bytes // 4), dtype=np.int64).astype(np.int32)
    live = _masks(N, seed=5)["random 50 % dead"]
    _new, old = compact_ref.plan(live)
    old_d = _up(old, dev)
    want = _up(compact_ref.rows_in_place(T, old), dev)
    flat = torch.full((N * row_bytes // 4 + 8,), SENTINEL, dtype=torch.int32, device=dev)
    shifted = flat[1:1 + N * row_bytes // 4].view(N, row_bytes // 4)
    assert shifted.data_ptr() % 16 == 4
    shifted.copy_(_up(T, dev))
    out = torch.full((old.size * row_bytes // 4 + 8,), SENTINEL, dtype=torch.int32, device=dev)
    _rows_raw(shifted, out.data_ptr() + 4, N, row_bytes, old_d, old.size, 0, dev)
    assert torch.equal(out[1:1 + old.size * row_bytes // 4].view(old.size, -1), want[:old.size])
    assert out[0] == SENTINEL and (out[1 + old.size * row_bytes // 4:] == SENTINEL).all()
    _rows_raw(shifted, shifted, N, row_bytes, old_d, old.size, 64, dev)
    assert torch.equal(shifted, want) and flat[0] == SENTINEL and (flat[1 + N * row_bytes // 4:] == SENTINEL).all()


def test_rows_in_place_past_2_32_bytes(dev):
    """1 150 000 rows of 4096 bytes (4.7 GB), every 7th dead: byte offsets past 2^32 in the gather, the bounce and the scatter.  Every
    row carries its old row number in its first word and a function of it in another."""
    N, W = 1_150_000, 1024
    need = N * W * 4 + (1 << 30)
    free = torch.cuda.mem_get_info(dev)[0]
    if free < need:
        pytest.skip(f"needs {need >> 20} MiB of free device memory, the device has {free >> 20} MiB free")
    t = torch.empty((N, W), dtype=torch.int32, device=dev)
    row = torch.arange(N, dtype=torch.int32, device=dev)
    t[:, 0] = row
    t[:, W - 1] = row * 7 + 3
    live = torch.ones(N, dtype=torch.bool, device=dev)
    live[6::7] = False
    plan = ops.compact_plan(ops.LiveRows.from_bool(live))
    want_old = torch.nonzero(live).flatten().to(torch.int32)
    assert plan.n_new == int(want_old.numel()) and torch.equal(plan.old_id, want_old)
    assert N * W * 4 > 2 ** 32 and int(want_old[-1]) * W * 4 > 2 ** 32      # the table, and the sources of the last rows moved
    out = plan.rows(t)
    assert out.data_ptr() == t.data_ptr() and out.shape == (plan.n_new, W)
    assert torch.equal(out[:, 0], want_old) and torch.equal(out[:, W - 1], want_old * 7 + 3)
    assert torch.equal(t[plan.n_new:, 0], row[plan.n_new:]) and torch.equal(t[plan.n_new:, W - 1], row[plan.n_new:] * 7 + 3)


# ------------------------------------------------------------------------------------------------------------------- ids, bitmaps
def test_ids_remap_matches_the_restatement(dev):
    N = 20_011
    live = _masks(N)["random 50 % dead"]
    new_id, old = compact_ref.plan(live)
    new_d = _up(new_id, dev)
    rng = np.random.default_rng(4)
    dead = np.nonzero(~live)[0]
    clean = np.concatenate([rng.choice(old, 5000), np.full(300, -1), [-5, -2 ** 31]]).astype(np.int32)
    dirty = np.concatenate([clean, rng.choice(dead, 40), [N, N + 1, 2 ** 31 - 1]]).astype(np.int32)
    for name, ids in (("live ids and padding", clean), ("with dead and out-of-range ids", dirty), ("one dead id", dead[:1].astype(np.int32)),
                      ("the last row", np.array([N - 1], np.int32))):
        ids = rng.permutation(ids)
        want, want_st = compact_ref.remap(new_id, ids)
        src = _up(ids, dev)
        out = torch.full((ids.size + 4,), SENTINEL, dtype=torch.int32, device=dev)
        st = torch.full((2,), SENTINEL, dtype=torch.int32, device=dev)
        assert lib().gdr_ids_remap(ptr(new_d), N, ptr(src), ptr(out), ids.size, ptr(st), stream_ptr()) == 0, lib().gdr_last_error()
        assert np.array_equal(out[:ids.size].cpu().numpy(), want) and (out[ids.size:] == SENTINEL).all(), name
        assert st.tolist() == [want_st, SENTINEL], name
        assert lib().gdr_ids_remap(ptr(new_d), N, ptr(src), ptr(src), ids.size, ptr(st), stream_ptr()) == 0      # out_ids aliases ids
        assert np.array_equal(src.cpu().numpy(), want) and st.tolist() == [want_st, SENTINEL], name + ", aliased"
    st.fill_(7)
    assert lib().gdr_ids_remap(ptr(new_d), N, None, None, 0, ptr(st), stream_ptr()) == 0 and st.tolist() == [0, 7]   # n = 0 clears the word
    # through ops: int64 results keep their shape and dtype; strict raises, strict=False maps to -1
    plan = ops.compact_plan(ops.LiveRows.from_bool(_up(live, dev)))
    assert np.array_equal(plan.new_id.cpu().numpy(), new_id) and np.array_equal(plan.old_id.cpu().numpy(), old)
    res = _up(clean[:5300].astype(np.int64).reshape(53, 100), dev)
    got = plan.ids(res)
    assert got.dtype == torch.int64 and got.shape == res.shape
    assert np.array_equal(got.cpu().numpy().reshape(-1), compact_ref.remap(new_id, clean[:5300])[0])
    bad = _up(np.array([int(old[0]), int(dead[0]), 2 ** 40, -1], np.int64), dev)
    with pytest.raises(_ffi.GdrError, match="dead row"):
        plan.ids(bad)
    assert plan.ids(bad, strict=False).tolist() == [0, -1, -1, -1]


@pytest.mark.parametrize("B", [1, 5])
def test_rowmask_compact_matches_the_repacked_bits(dev, B):
    for N in (1, 33, 64, 65, 1000, 20_011):
        rng = np.random.default_rng(N + B)
        for name, live in _masks(N, seed=B).items():
            _new, old = compact_ref.plan(live)
            n_live = old.size
            allowed = rng.random((B, N)) < 0.4
            W, Wn = (N + 31) // 32, (n_live + 31) // 32
            si, so = W + 3, Wn + 2
            win = np.full((B, si), -1, np.int32)                               # all ones behind every input bitmap
            win[:, :W] = compact_ref.pack(allowed)
            if N % 32:
                win[:, W - 1] |= np.int32(-1 << (N % 32))                      # and every bit past N
            wout = torch.full((B, so), SENTINEL, dtype=torch.int32, device=dev)
            win_d, old_d = _up(win, dev), _up(old, dev)
            rc = lib().gdr_rowmask_compact(ptr(win_d), si, B, N, ptr(old_d) if n_live else None, n_live, ptr(wout), so, stream_ptr())
            assert rc == 0, lib().gdr_last_error().decode()
            what = f"B={B}, N={N}, {name}"
            assert np.array_equal(wout[:, :Wn].cpu().numpy(), compact_ref.rowmask(allowed, old).reshape(B, Wn)), what   # pad bits are 0
            assert (wout[:, Wn:] == SENTINEL).all(), what + ": a word past ceil(n_live / 32) was written"
    # through ops
    N = 1000
    live = _masks(N)["random 50 % dead"]
    allowed = np.random.default_rng(1).random((B, N)) < 0.3
    plan = ops.compact_plan(ops.LiveRows.from_bool(_up(live, dev)))
    qr = plan.query_rows(ops.QueryRows.from_bool(_up(allowed, dev)))
    assert (qr.B, qr.n) == (B, plan.n_new) and np.array_equal(qr.to_bool().cpu().numpy(), allowed[:, live])


# ------------------------------------------------------------------------------------------------------------------- memory contract
@pytest.mark.parametrize("fill", [0x00, 0xFF, 0x5A])
def test_memory_contract_of_the_four_calls(dev, fill):
    """Guard bands around every buffer, a poisoned workspace of exactly the declared size, a non-default stream, a second run on the
    warm workspace, and inputs followed by values that would change the answer if they were read."""
    N, row_bytes, B, chunk = 20_011, 200, 3, 300
    rng = np.random.default_rng(fill)
    live = rng.random(N) >= 0.4
    want_new, want_old = compact_ref.plan(live)
    n_live = want_old.size
    W, Wn = (N + 31) // 32, (n_live + 31) // 32
    T = rng.integers(-2 ** 31, 2 ** 31, (N, row_bytes // 4), dtype=np.int64).astype(np.int32)
    allowed = rng.random((B, N)) < 0.5
    ids = np.concatenate([rng.choice(want_old, 3000), [-1, -1]]).astype(np.int32)
    ones = lambda n: torch.full((n,), -1, dtype=torch.int32)   # noqa: E731
    words, h_words = guarded_input(torch.from_numpy(_dirty(compact_ref.pack(live), N)), tail=ones(64))      # live rows behind the bitmap
    win, h_win = guarded_input(torch.from_numpy(compact_ref.pack(allowed)), tail=ones(64))
    ids_d, h_ids = guarded_input(torch.from_numpy(ids), tail=torch.from_numpy(want_old[:64].copy()))           # valid ids behind the list
    src, h_src = guarded_input(torch.from_numpy(T), tail=torch.from_numpy(T[:4].copy()))
    new_id, h_new = guarded((N,), torch.int32, dev)
    old_id, h_old = guarded((n_live,), torch.int32, dev)
    status, h_st = guarded((1,), torch.int32, dev)
    rstatus, h_rst = guarded((1,), torch.int32, dev)
    out_ids, h_oi = guarded((ids.size,), torch.int32, dev)
    out_rows, h_or = guarded((n_live, row_bytes // 4), torch.int32, dev)
    inplace, h_ip = guarded((N, row_bytes // 4), torch.int32, dev)
    wout, h_wo = guarded((B, Wn), torch.int32, dev)
    plan_ws, h_pws = poisoned_workspace(lib().gdr_rows_compact_plan_workspace_bytes(N), fill, dev)
    rows_ws, h_rws = poisoned_workspace(lib().gdr_rows_compact_workspace_bytes(row_bytes, chunk), fill, dev)
    st = torch.cuda.Stream(device=dev)
    st.wait_stream(torch.cuda.current_stream())
    l = lib()
    with torch.cuda.stream(st):
        for run in range(2):                                                   # the second run meets the workspaces as the first left them
            inplace.copy_(src)
            assert l.gdr_rows_compact_plan(ptr(words), N, n_live, ptr(new_id), ptr(old_id), ptr(status), ptr(plan_ws), plan_ws.numel(),
                                           stream_ptr()) == 0, l.gdr_last_error()
            assert l.gdr_rows_compact(ptr(src), ptr(out_rows), N, row_bytes, ptr(old_id), n_live, 0, None, 0, stream_ptr()) == 0, l.gdr_last_error()
            assert l.gdr_rows_compact(ptr(inplace), ptr(inplace), N, row_bytes, ptr(old_id), n_live, chunk, ptr(rows_ws), rows_ws.numel(),
                                      stream_ptr()) == 0, l.gdr_last_error()
            assert l.gdr_ids_remap(ptr(new_id), N, ptr(ids_d), ptr(out_ids), ids.size, ptr(rstatus), stream_ptr()) == 0, l.gdr_last_error()
            assert l.gdr_rowmask_compact(ptr(win), W, B, N, ptr(old_id), n_live, ptr(wout), Wn, stream_ptr()) == 0, l.gdr_last_error()
            st.synchronize()
            what = f"fill={fill:#x}, run {run}"
            assert status.tolist() == [0] and rstatus.tolist() == [0], what
            assert np.array_equal(new_id.cpu().numpy(), want_new) and np.array_equal(old_id.cpu().numpy(), want_old), what
            assert np.array_equal(out_rows.cpu().numpy(), compact_ref.rows(T, want_old)), what
            assert np.array_equal(inplace.cpu().numpy(), compact_ref.rows_in_place(T, want_old)), what
            assert np.array_equal(out_ids.cpu().numpy(), compact_ref.remap(want_new, ids)[0]), what
            assert np.array_equal(wout.cpu().numpy(), compact_ref.rowmask(allowed, want_old)), what
            for h, name in ((h_new, "out_new_id"), (h_old, "out_old_id"), (h_st, "out_status"), (h_rst, "remap status"), (h_oi, "out_ids"),
                            (h_or, "dst"), (h_ip, "the in-place table"), (h_wo, "words_out"), (h_pws, "the plan's workspace"),
                            (h_rws, "the mover's workspace")):
                h.check(f"{what}: {name}")
            for h, name in ((h_words, "live_words"), (h_win, "words_in"), (h_ids, "ids"), (h_src, "src")):
                h.unchanged(f"{what}: {name}")
    torch.cuda.current_stream().wait_stream(st)


# ------------------------------------------------------------------------------------------------------------------- graph capture
def test_plan_move_and_remap_in_a_captured_graph_follow_the_bitmap(dev):
    N, row_bytes, chunk = 20_011, 256, 1000
    rng = np.random.default_rng(9)
    T = rng.integers(-2 ** 31, 2 ** 31, (N, row_bytes // 4), dtype=np.int64).astype(np.int32)
    n_live = 12_000
    lives = []
    for _ in range(2):
        live = np.zeros(N, bool)
        live[rng.choice(N, n_live, replace=False)] = True
        lives.append(live)
    ids = np.nonzero(lives[0] & lives[1])[0][:500].astype(np.int32)           # live under both bitmaps
    words = _up(compact_ref.pack(lives[0]), dev)
    T0, t, ids_d = _up(T, dev), torch.empty((N, row_bytes // 4), dtype=torch.int32, device=dev), _up(ids, dev)
    new_id = torch.empty(N, dtype=torch.int32, device=dev)
    old_id = torch.empty(n_live, dtype=torch.int32, device=dev)
    out_ids = torch.empty(ids.size, dtype=torch.int32, device=dev)
    status = torch.empty(2, dtype=torch.int32, device=dev)
    pws = torch.empty(lib().gdr_rows_compact_plan_workspace_bytes(N), dtype=torch.uint8, device=dev)
    rws = torch.empty(lib().gdr_rows_compact_workspace_bytes(row_bytes, chunk), dtype=torch.uint8, device=dev)
    l = lib()

    def call():
        t.copy_(T0)
        assert l.gdr_rows_compact_plan(ptr(words), N, n_live, ptr(new_id), ptr(old_id), ptr(status), ptr(pws), pws.numel(), stream_ptr()) == 0
        assert l.gdr_rows_compact(ptr(t), ptr(t), N, row_bytes, ptr(old_id), n_live, chunk, ptr(rws), rws.numel(), stream_ptr()) == 0
        assert l.gdr_ids_remap(ptr(new_id), N, ptr(ids_d), ptr(out_ids), ids.size, ptr(status[1:]), stream_ptr()) == 0

    def check(live, what):
        torch.cuda.synchronize()
        want_new, want_old = compact_ref.plan(live)
        assert status.tolist() == [0, 0], what
        assert np.array_equal(new_id.cpu().numpy(), want_new) and np.array_equal(old_id.cpu().numpy(), want_old), what
        assert np.array_equal(t.cpu().numpy(), compact_ref.rows_in_place(T, want_old)), what
        assert np.array_equal(out_ids.cpu().numpy(), want_new[ids]), what

    warm = torch.cuda.Stream(device=dev)
    warm.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(warm):
        call()                                                                # eager; also the one run a capture needs first
    torch.cuda.current_stream().wait_stream(warm)
    check(lives[0], "eager")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for o in (new_id, old_id, out_ids, status):
        o.zero_()
    g.replay()
    check(lives[0], "graph replay")
    words.copy_(_up(compact_ref.pack(lives[1]), dev))                         # another bitmap with the same n_live
    g.replay()
    check(lives[1], "graph replay after the bitmap was rewritten")


# ------------------------------------------------------------------------------------------------------------------- ops
def test_compact_plan_checks_the_count_and_identity_plans_launch_nothing(dev):
    N = 1000
    live = _masks(N)["random 50 % dead"]
    L = ops.LiveRows.from_bool(_up(live, dev))
    L.count += 1
    with pytest.raises(_ffi.GdrError, match="count"):
        ops.compact_plan(L)
    full = ops.LiveRows.from_bool(torch.ones(N, dtype=torch.bool, device=dev))
    plan = ops.compact_plan(full)
    assert plan.identity and (plan.n_old, plan.n_new) == (N, N) and torch.equal(plan.new_id, torch.arange(N, dtype=torch.int32, device=dev))
    t = torch.arange(N * 3, dtype=torch.float32, device=dev).view(N, 3)
    ids = torch.arange(10, dtype=torch.int64, device=dev)
    qr = ops.QueryRows.from_bool(_up(live[None], dev))
    n0 = lib().gdr_launch_count()
    assert plan.rows(t) is t and plan.ids(ids) is ids and plan.query_rows(qr) is qr
    assert lib().gdr_launch_count() == n0
    assert plan.live_rows().count == N
    # rows(): dtypes whose row is a multiple of 4 bytes — bf16 pairs, int64 — and a refusal for one that is not
    plan = ops.compact_plan(ops.LiveRows.from_bool(_up(live, dev)))
    assert not plan.identity and plan.n_new == int(live.sum())
    for t in (torch.randn((N, 6), device=dev).bfloat16(), torch.arange(N * 5, device=dev).view(N, 5), torch.randn((N, 2, 3), device=dev)):
        want = t[_up(live, dev)]
        out = plan.rows(t.clone(), out=torch.empty_like(t))
        assert torch.equal(out, want)
        got = plan.rows(t)
        assert got.data_ptr() == t.data_ptr() and torch.equal(got, want)
    with pytest.raises(_ffi.GdrError, match="multiples of 4"):
        plan.rows(torch.zeros((N, 3), dtype=torch.bfloat16, device=dev))
    with pytest.raises(_ffi.GdrError, match="contiguous"):
        plan.rows(torch.zeros((N + 1, 4), device=dev))
    L2 = plan.live_rows()
    assert L2.n == L2.count == plan.n_new and bool(L2.to_bool().all())


# ------------------------------------------------------------------------------------------------------------------- the retriever
def _args(V, R=4):
    return types.SimpleNamespace(num_return_sequences=R, output_vocab_size=V, max_output_length=GDRConfig.tiny().max_output_length,
                                 length_penalty=0.8, kary=V, position=1, score_rate=[0, 1.0], loss_func="tanh")


@pytest.fixture(scope="module")
def tiny_setup(dev):
    """The tiny model over V*V clusters of 60 documents (2160 documents, d = 64), one batch of 4 queries for the two-stage step, 6
    queries for the corpus search, and a token table."""
    from gdr_amd.modeling import GDRModel
    cfg = GDRConfig.tiny()
    sd = synth.make_state_dict(cfg, seed=1234)
    V = cfg.output_vocab_size
    names = ["-".join(str(x) for x in synth.cluster_digits(c, 2, V)) for c in range(V * V)]
    csz = 60
    N0 = len(names) * csz
    assert cfg.d_model == 64 and N0 >= 2000
    D0 = synth.make_corpus(N0, cfg.d_model, cluster_size=csz, seed=8) * np.float32(0.05)
    idx = codec.ClusterIndex(names, (np.arange(len(names) + 1) * csz).astype(np.int32), np.arange(N0, dtype=np.int32))
    full = codec.Trie.from_docids(names, V)
    model = GDRModel(cfg, sd, dev, trie=full, prefix_trie=full)
    ids, mask = synth.make_tokens(4, L=12, vocab_hi=cfg.vocab_size, seed=5, min_len=3)
    batch = {"source_ids": torch.from_numpy(ids).to(dev), "source_mask": torch.from_numpy(mask).to(dev)}
    Q, _ = synth.make_queries(D0, 6, seed=3)
    tok, msk = synth.make_tokens(N0 + 16, L=10, vocab_hi=cfg.vocab_size, seed=11)
    return types.SimpleNamespace(cfg=cfg, V=V, idx=idx, D0=D0, model=model, batch=batch, csz=csz, N0=N0, Q=Q, Qd=torch.from_numpy(Q).to(dev),
                                 tok=torch.from_numpy(tok).to(dev), msk=torch.from_numpy(msk).to(dev))


def _turned_over(s, dev, **kw):
    """A retriever that has lived: 8 documents added, a few hundred removed (every query's best documents among them), a third
    of those restored by an update."""
    from gdr_amd.modeling import GDRRetriever
    N0 = s.N0
    r = GDRRetriever(s.model, torch.from_numpy(s.D0).to(dev), s.idx, _args(s.V), doc_tokens=(s.tok[:N0].clone(), s.msk[:N0].clone()), **kw)
    base = r.validation_step_i(s.batch)["doc_id_tensor"].cpu().numpy()
    _v, top = r.search(s.Qd, 20)
    X = torch.from_numpy((s.D0[5:13] * np.float32(1.01)).astype(np.float32)).to(dev)
    new_ids, _cl = r.add_documents(X, tokens=(s.tok[N0:N0 + 8], s.msk[N0:N0 + 8]))
    gone = np.unique(np.concatenate([top.cpu().numpy()[:, :5].reshape(-1), base[base >= 0][:6], np.arange(0, N0, 7), np.arange(N0 - 40, N0),
                                     new_ids[:2]]))
    r.remove_documents(gone)
    back = gone[::3]
    back = back[back < N0]
    r.update_documents(back, torch.from_numpy(s.D0[back]).to(dev), tokens=(s.tok[back], s.msk[back]))
    return r, np.setdiff1d(gone, back)


def _filters(s, r, dead, dev):
    """(wide, narrow) QueryRows over r's rows: half of the corpus per query; about 40 rows per query, dead ones among them."""
    N = r.doc_embed.shape[0]
    rng = np.random.default_rng(N)
    B = s.Qd.shape[0]
    wide = rng.random((B, N)) < 0.5
    narrow = np.zeros((B, N), bool)
    for q in range(B):
        narrow[q, rng.choice(N, 40, replace=False)] = True
        narrow[q, dead[q::B][:5]] = True
    return wide, narrow


def _mapped(plan, ids):
    return plan.ids(ids.to(plan.device)).cpu()


@pytest.mark.parametrize("form", ["device_candidates", "host_candidates", "search_prefilter"])
def test_compact_documents_end_to_end(dev, tiny_setup, form):
    from gdr_amd.modeling import GDRRetriever
    s = tiny_setup
    kw = {"device_candidates": dict(), "host_candidates": dict(device_candidates=False), "search_prefilter": dict(search_prefilter=True)}[form]
    r, dead = _turned_over(s, dev, **kw)
    k = 20
    wide, narrow = _filters(s, r, dead, dev)
    a_w, a_n = ops.QueryRows.from_bool(_up(wide, dev)), ops.QueryRows.from_bool(_up(narrow, dev))
    v0, i0 = r.search(s.Qd, k)
    vw, iw = r.search(s.Qd, k, allowed=a_w, gather=False)                     # the dense masked route
    vn, i_n = r.search(s.Qd, k, allowed=a_n)                                  # the gather route
    step0 = r.validation_step_i(s.batch)
    n_old = r.doc_embed.shape[0]
    live = r.live_rows.to_bool().cpu().numpy()
    assert not live[dead].any() and live.sum() == n_old - dead.size
    D_old, tok_old, msk_old = r.doc_embed.cpu().numpy(), r.doc_tokens[0].cpu().numpy(), r.doc_tokens[1].cpu().numpy()
    offs_old, mem_old = r.index.offsets.copy(), r.index.members.copy()
    buf_ptr, tok_ptr = r._doc_buf.data_ptr(), r.doc_tokens[0].data_ptr()
    assert r.doc_embed.data_ptr() == buf_ptr
    cent = r._centroids.centroids.clone()
    want_new, want_old = compact_ref.plan(live)

    plan = r.compact_documents()
    n_new = plan.n_new
    assert not plan.identity and (plan.n_old, n_new) == (n_old, int(live.sum()))
    assert np.array_equal(plan.new_id.cpu().numpy(), want_new) and np.array_equal(plan.old_id.cpu().numpy(), want_old)
    # the rows
    assert r.doc_embed.shape[0] == n_new and r.doc_embed.data_ptr() == buf_ptr == r._doc_buf.data_ptr() and r._doc_buf.shape[0] >= n_old
    assert np.array_equal(r.doc_embed.cpu().numpy().view(np.uint32), compact_ref.rows(D_old, want_old).view(np.uint32))
    assert r.doc_tokens[0].data_ptr() == tok_ptr and r.doc_tokens[0].shape[0] == n_new
    assert np.array_equal(r.doc_tokens[0].cpu().numpy(), compact_ref.rows(tok_old, want_old))
    assert np.array_equal(r.doc_tokens[1].cpu().numpy(), compact_ref.rows(msk_old, want_old))
    # the index: the old one with members mapped, in the same order — a fresh index built from the restatement
    assert np.array_equal(r.index.offsets, offs_old) and np.array_equal(r.index.members, compact_ref.index_members(mem_old, want_new))
    assert list(r.index.names) == list(s.idx.names)
    dci = r._device_index()
    assert (dci is not None) == (form != "host_candidates")
    if dci is not None:
        assert np.array_equal(dci.members[:dci.n_members].cpu().numpy(), r.index.members)
        assert np.array_equal(dci.offsets.cpu().numpy(), offs_old)
    L = r.live_rows
    assert L.count == L.n == n_new == r.doc_embed.shape[0] and bool(L.to_bool().all())
    assert torch.equal(r._centroids.centroids, cent)
    # the corpus search: the old ids mapped through new_id, the values bit for bit (d = 64: the tiled core)
    v1, i1 = r.search(s.Qd, k)
    assert torch.equal(i1.cpu(), _mapped(plan, i0)) and torch.equal(v1, v0)
    uv, ui = ops.sim_topk(s.Qd, r.doc_embed, k)                               # nothing is dead: the unmasked call over the new corpus
    assert torch.equal(ui.to(torch.int64), i1)
    rv, ri = live_ref.topk(live_ref.scores(s.Q, r.doc_embed.cpu().numpy()), np.ones(n_new, bool), k)
    order_insensitive_topk_match(rv, ri, v1.cpu().numpy(), i1.cpu().numpy(), TOL)
    b_w, b_n = plan.query_rows(a_w), plan.query_rows(a_n)
    assert np.array_equal(b_w.to_bool().cpu().numpy(), wide[:, live]) and np.array_equal(b_n.to_bool().cpu().numpy(), narrow[:, live])
    v2, i2 = r.search(s.Qd, k, allowed=b_w, gather=False)
    assert torch.equal(i2.cpu(), _mapped(plan, iw)) and torch.equal(v2, vw)
    v3, i3 = r.search(s.Qd, k, allowed=b_n)
    assert torch.equal(i3.cpu(), _mapped(plan, i_n)) and torch.equal(v3, vn)
    assert int((i_n >= 0).sum()) > 0 and int((i_n < 0).sum()) == 0
    if form == "search_prefilter":
        P = r._prefiltered
        assert P is not None and P.D.data_ptr() == r.doc_embed.data_ptr() and P.D16.shape[0] == n_new
        assert torch.equal(P.D16.view(torch.int16), ops.to_bf16(r.doc_embed).view(torch.int16)), "the image is not a fresh image of the new doc_embed"
    # the two-stage step: the same lists with ids mapped and bit-identical values; and the step of a fresh retriever over the restatement
    step1 = r.validation_step_i(s.batch)
    assert torch.equal(step1["doc_id_tensor"].cpu().to(torch.int64), _mapped(plan, step0["doc_id_tensor"].to(torch.int64)))
    assert torch.equal(step1["rerank_values"], step0["rerank_values"])
    assert int((step0["doc_id_tensor"] >= 0).sum()) > 0
    fresh = GDRRetriever(s.model, _up(compact_ref.rows(D_old, want_old), dev),
                         s.idx.with_csr(offs_old, compact_ref.index_members(mem_old, want_new)), _args(s.V)).validation_step_i(s.batch)
    assert torch.equal(fresh["doc_id_tensor"].cpu(), step1["doc_id_tensor"].cpu()) and torch.equal(fresh["rerank_values"], step1["rerank_values"])

    # life goes on: a second removal and compaction compose to one plan over the union
    g2 = np.unique(np.concatenate([i1.cpu().numpy()[:, 0], np.arange(3, n_new, 11)]))
    r.remove_documents(g2)
    plan2 = r.compact_documents()
    union = live.copy()
    union[want_old[g2]] = False
    assert np.array_equal(compact_ref.compose(want_new, plan2.new_id.cpu().numpy()), compact_ref.plan(union)[0])
    assert np.array_equal(r.doc_embed.cpu().numpy().view(np.uint32), D_old[union].view(np.uint32))
    assert np.array_equal(r.doc_tokens[0].cpu().numpy(), tok_old[union])
    # and an addition appends behind the live rows, in the same backing buffer, into the clusters it would have joined before
    X = torch.from_numpy((s.D0[100:104] * np.float32(0.99)).astype(np.float32)).to(dev)
    want_cl = r._centroids.assign(X).cpu().numpy()
    n2 = plan2.n_new
    new_ids, cl = r.add_documents(X, tokens=(s.tok[s.N0 + 8:s.N0 + 12], s.msk[s.N0 + 8:s.N0 + 12]))
    assert new_ids.tolist() == list(range(n2, n2 + 4)) and np.array_equal(cl, want_cl)
    assert r.doc_embed.data_ptr() == buf_ptr and r.doc_tokens[0].data_ptr() == tok_ptr and r.doc_embed.shape[0] == n2 + 4
    assert r.live_rows.count == r.live_rows.n == n2 + 4
    v4, i4 = r.search(s.Qd, k)
    rv, ri = live_ref.topk(live_ref.scores(s.Q, r.doc_embed.cpu().numpy()), np.ones(n2 + 4, bool), k)
    order_insensitive_topk_match(rv, ri, v4.cpu().numpy(), i4.cpu().numpy(), TOL)
    if form == "search_prefilter":
        assert torch.equal(r._prefiltered.D16.view(torch.int16), ops.to_bf16(r.doc_embed).view(torch.int16))


def test_compacted_search_on_the_fp32_stream_kernels(dev):
    """B = 4, d = 128: the fp32 stream kernels, whose bits depend on the tile a row sits in (tests/test_gpu_live_search.py explains
    why), so the compacted search is held to oracle/parity_rules.py's rule, not to bit equality."""
    from gdr_amd.modeling import GDRRetriever
    V, csz, d, k, B = 30, 3, 128, 10, 4
    names = ["-".join(str(x) for x in synth.cluster_digits(c, 2, V)) for c in range(V * V)]
    N0 = len(names) * csz
    D0 = synth.make_corpus(N0, d, cluster_size=csz, seed=8)
    Q, _ = synth.make_queries(D0, B, seed=3)
    Qd = torch.from_numpy(Q).to(dev)
    idx = codec.ClusterIndex(names, (np.arange(len(names) + 1) * csz).astype(np.int32), np.arange(N0, dtype=np.int32))
    r = GDRRetriever(None, torch.from_numpy(D0).to(dev), idx, _args(V))
    _v, top = r.search(Qd, k)
    gone = np.unique(np.concatenate([top.cpu().numpy()[:, :3].reshape(-1), np.arange(0, N0, 5)]))
    r.remove_documents(gone)
    v0, i0 = r.search(Qd, k)
    plan = r.compact_documents()
    v1, i1 = r.search(Qd, k)
    order_insensitive_topk_match(v0.cpu().numpy(), _mapped(plan, i0).numpy(), v1.cpu().numpy(), i1.cpu().numpy(), TOL)
    live = np.ones(N0, bool)
    live[gone] = False
    rv, ri = live_ref.topk(live_ref.scores(Q, D0[live]), np.ones(int(live.sum()), bool), k)
    order_insensitive_topk_match(rv, ri, v1.cpu().numpy(), i1.cpu().numpy(), TOL)
    assert np.array_equal(r.doc_embed.cpu().numpy().view(np.uint32), D0[live].view(np.uint32))


def test_centroids_frozen_after_a_compaction_have_the_bits_of_those_frozen_before(dev, tiny_setup):
    """On a retriever that has not frozen yet: its index omits a few hundred rows from the start."""
    from gdr_amd.modeling import GDRRetriever
    s = tiny_setup
    gone = np.unique(np.concatenate([np.arange(0, s.N0, 7), np.arange(300, 340)]))
    offs, mem, _n = lifecycle_ref.remove(s.idx.offsets, s.idx.members, gone)
    partial = s.idx.with_csr(offs, mem)
    D = torch.from_numpy(s.D0).to(dev)
    before = ops.FrozenCentroids(D, partial)
    r = GDRRetriever(None, D.clone(), partial, _args(s.V))
    plan = r.compact_documents()
    assert plan.n_new == s.N0 - gone.size and getattr(r, "_centroids", None) is None
    after = r._freeze_centroids()
    assert torch.equal(after.centroids.view(torch.int32), before.centroids.view(torch.int32)) and torch.equal(after.counts, before.counts)
    cent, counts = expand_ref.centroids(s.D0, offs, mem)
    assert np.array_equal(after.centroids.cpu().numpy().view(np.uint32), cent.view(np.uint32))


def test_identity_and_refusals_change_nothing(dev, tiny_setup):
    from gdr_amd.modeling import GDRRetriever
    s = tiny_setup
    D = torch.from_numpy(s.D0).to(dev)
    r = GDRRetriever(None, D.clone(), s.idx, _args(s.V), doc_tokens=(s.tok[:s.N0].clone(), s.msk[:s.N0].clone()))
    p_d, p_t, live0 = r.doc_embed.data_ptr(), r.doc_tokens[0].data_ptr(), r.live_rows
    plan = r.compact_documents()
    assert plan.identity and plan.n_new == s.N0
    assert r.doc_embed.data_ptr() == p_d and r.doc_tokens[0].data_ptr() == p_t and r.live_rows is live0 and r.index is s.idx
    assert torch.equal(r.doc_embed, D) and torch.equal(r.doc_tokens[0], s.tok[:s.N0]) and torch.equal(r.doc_tokens[1], s.msk[:s.N0])
    sh = GDRRetriever(None, D, s.idx, _args(s.V), sharded=types.SimpleNamespace(D=D))
    bf = GDRRetriever(None, D.to(torch.bfloat16), s.idx, _args(s.V))
    for q, word in ((sh, "sharded"), (bf, "bf16")):
        E = q.doc_embed.clone()
        with pytest.raises(_ffi.GdrError, match=word):
            q.compact_documents()
        assert q.index is s.idx and torch.equal(q.doc_embed, E) and getattr(q, "_live", None) is None and not hasattr(q, "_dci")
    # a member list that names a dead row: GdrError, and the device list is what it was
    dci = ops.DeviceClusterIndex(s.idx, dev, s.V, position=1, kary=s.V)
    live = np.ones(s.N0, bool)
    live[7] = False
    bad = ops.compact_plan(ops.LiveRows.from_bool(_up(live, dev)))
    with pytest.raises(_ffi.GdrError, match="not a live row"):
        dci.compact(bad)
    assert np.array_equal(dci.members[:dci.n_members].cpu().numpy(), s.idx.members)
