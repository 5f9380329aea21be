"""Corpus search over live rows, host side: the workspace sizing and the pre-launch errors of gdr_sim_topk's
GDR_SIM_LIVE_MASK mode, the pinned ABI, ops.LiveRows on the CPU and the numpy restatement (tests/live_ref.py).  Needs no GPU."""
import ctypes as C
import hashlib

import numpy as np
import pytest
import torch

import live_ref
from gdr_amd import _ffi, ops

# (B, N, k) -> gdr_sim_topk_workspace_bytes(B, N, d, k, flags) for flags 0 and GDR_SIM_EXHAUSTIVE as they were before the mode existed
PLAIN = {
    (8, 70_001, 10): (640_256, 4_613_376),
    (512, 320_000, 100): (130_615_296, 1_310_787_584),
    (4, 1000, 10): (99_072, 99_072),
    (40, 2_800_003, 8192): (239_785_216, 896_046_336),
}


def test_flag_value_and_pinned_abi():
    assert _ffi.SIM_LIVE_MASK == 4 and _ffi.SIM_LIVE_MASK & (_ffi.SIM_EXHAUSTIVE | _ffi.SIM_NO_STREAM) == 0
    assert _ffi.lib().gdr_abi_version() == 9 == _ffi.ABI_VERSION
    # the mode is a flag of existing calls: no entry point was added and none changed its signature
    name = lambda t: getattr(t, "__name__", str(t))   # noqa: E731
    text = ";".join(f"{k}:{name(r)}({','.join(name(a) for a in args)})" for k, (r, args) in sorted(_ffi.SIGNATURES.items()))
    assert len(_ffi.SIGNATURES) == 75
    assert hashlib.sha256(text.encode()).hexdigest() == "290bf61378c8afa411523c3af82231a508b23b22da2603b6645954cc9845c9c2"


@pytest.mark.parametrize("B,N,k", list(PLAIN))
def test_workspace_is_the_plain_size_plus_the_bitmap(B, N, k):
    """Fails without the feature: bit 4 of flags was ignored, so the flagged size was the plain one."""
    l = _ffi.lib()
    for d in (64, 768):
        for extra, want in zip((0, _ffi.SIM_EXHAUSTIVE), PLAIN[(B, N, k)]):
            for more in (0, _ffi.SIM_NO_STREAM):
                plain = l.gdr_sim_topk_workspace_bytes(B, N, d, k, extra | more)
                assert plain == want, "the unflagged size moved"
                assert l.gdr_sim_topk_workspace_bytes(B, N, d, k, extra | more | _ffi.SIM_LIVE_MASK) - plain == live_ref.mask_bytes(N)
    assert l.gdr_sim_topk_workspace_bytes(0, N, 64, k, _ffi.SIM_LIVE_MASK) == 0


def test_flagged_call_refuses_a_workspace_without_room_for_the_bitmap_before_any_launch():
    """The pointers are never dereferenced.  A buffer of the UNFLAGGED size is GDR_ENOSPC at every shape — also where this k's own
    layout dips below the unflagged answer (512 x 320 000, k = 100) and the bitmap would happen to fit."""
    l = _ffi.lib()
    p, ws = C.c_void_p(256), C.c_void_p(4096)
    for (B, N, k) in PLAIN:
        for fn in (l.gdr_sim_topk, l.gdr_sim_topk_bf16):
            for more in (0, _ffi.SIM_EXHAUSTIVE, _ffi.SIM_NO_STREAM):
                flags = _ffi.SIM_LIVE_MASK | more
                plain = l.gdr_sim_topk_workspace_bytes(B, N, 64, k, more)
                need = l.gdr_sim_topk_workspace_bytes(B, N, 64, k, flags)
                for nbytes in (plain, need - 1):
                    assert fn(p, B, p, N, 64, k, 0, p, p, None, flags, ws, nbytes, None) == _ffi.GDR_ENOSPC, (B, N, k, flags, nbytes)
                    msg = l.gdr_last_error()
                    assert str(need).encode() in msg and str(nbytes).encode() in msg, msg
    # a misaligned workspace is refused whatever its size
    assert l.gdr_sim_topk(p, 8, p, 70_001, 64, 10, 0, p, p, None, _ffi.SIM_LIVE_MASK, C.c_void_p(4096 + 128), 1 << 30, None) == _ffi.GDR_EINVAL
    assert b"256-byte aligned" in l.gdr_last_error()


def test_header_documents_the_flag_and_the_unmasked_prefilter():
    import os
    from conftest import REPO
    text = open(os.path.join(REPO, "include", "gdr_hip.h")).read()
    assert "#define GDR_SIM_LIVE_MASK 4" in text
    assert "stays UNMASKED" in text


# ---------------------------------------------------------------------------------------------- ops.LiveRows (CPU device)
def test_live_rows_pack_set_clear_grow():
    rng = np.random.default_rng(0)
    for n in (1, 31, 32, 33, 64, 1000, 4097):
        x = rng.random(n) < 0.5
        x[-1] = True                                                      # the last row, bit (n - 1) % 32 (bit 31 at n = 32, 64)
        L = ops.LiveRows.from_bool(torch.from_numpy(x))
        assert L.n == n and L.count == int(x.sum()) and L.words.dtype == torch.int32 and L.words.numel() == -(-n // 32)
        assert np.array_equal(L.words.numpy(), live_ref.pack(x)), n
        assert np.array_equal(L.to_bool().numpy(), x)
    x = rng.random(1000) < 0.5
    L = ops.LiveRows.from_bool(torch.from_numpy(x))
    ids = np.concatenate([rng.choice(1000, 300, replace=False), [31, 63, 999, 31]])           # repeats, word boundaries
    assert L.set(ids) == int((~x[np.unique(ids)]).sum())
    x[ids] = True
    assert np.array_equal(L.words.numpy(), live_ref.pack(x)) and L.count == int(x.sum())
    assert L.set(ids) == 0 and np.array_equal(L.words.numpy(), live_ref.pack(x))
    ids = torch.from_numpy(np.concatenate([rng.choice(1000, 400), [0, 31, 32, 991]]))
    was = int(x[np.unique(ids.numpy())].sum())
    assert L.clear(ids) == was
    x[ids.numpy()] = False
    assert np.array_equal(L.words.numpy(), live_ref.pack(x)) and L.count == int(x.sum())
    L.grow(1100)
    x = np.concatenate([x, np.zeros(100, bool)])
    assert L.n == 1100 and np.array_equal(L.words.numpy(), live_ref.pack(x)) and L.count == int(x.sum())
    L.set(np.arange(1000, 1100, 3))
    x[1000:1100:3] = True
    assert np.array_equal(L.words.numpy(), live_ref.pack(x)) and L.count == int(x.sum())
    L.grow(5000)                                                          # beyond the backing buffer
    assert L.words.numel() == 157 and np.array_equal(L.to_bool().numpy(), np.concatenate([x, np.zeros(3900, bool)]))
    empty = ops.LiveRows(70, "cpu")
    assert empty.count == 0 and empty.words.numel() == 3 and not empty.to_bool().any()
    assert empty.set([]) == 0 and empty.clear([5]) == 0
    for bad in ([-1], [70]):
        with pytest.raises(_ffi.GdrError, match=r"\[0, 70\)"):
            empty.set(bad)
    with pytest.raises(_ffi.GdrError, match="grow"):
        empty.grow(69)


def test_sim_topk_validates_live_before_anything_runs():
    Q, D = torch.zeros(2, 8), torch.zeros(40, 8)
    with pytest.raises(_ffi.GdrError, match="CUDA"):
        ops.sim_topk(Q, D, 3, live=ops.LiveRows(40, "cpu"))


# ---------------------------------------------------------------------------------------------- the restatement
def test_restatement_on_hand_written_cases():
    S = np.array([[1.0, 5.0, 3.0, 5.0, 2.0, 4.0],
                  [0.0, 0.0, 0.0, 0.0, 0.0, 0.0]])
    live = np.array([1, 1, 1, 1, 0, 1], bool)
    v, i = live_ref.topk(S, live, 3)
    assert i.tolist() == [[1, 3, 5], [0, 1, 2]] and v.tolist() == [[5.0, 5.0, 4.0], [0.0, 0.0, 0.0]]   # ties: the lower id first
    v, i = live_ref.topk(S, np.array([1, 0, 1, 1, 0, 0], bool), 3, idx_offset=100)
    assert i.tolist() == [[103, 102, 100], [100, 102, 103]] and v[0].tolist() == [5.0, 3.0, 1.0]
    v, i = live_ref.topk(S, np.array([0, 0, 1, 0, 0, 1], bool), 4, idx_offset=7)                        # fewer than k live
    assert i.tolist() == [[12, 9, -1, -1], [9, 12, -1, -1]]
    assert v[0].tolist() == [4.0, 3.0, -np.inf, -np.inf]
    v, i = live_ref.topk(S, np.zeros(6, bool), 2)
    assert (i == -1).all() and np.isneginf(v).all()
    Q, D = np.array([[1.0, 2.0]], np.float32), np.array([[1, 0], [0, 1], [1, 1]], np.float32)
    assert live_ref.scores(Q, D).tolist() == [[1.0, 2.0, 3.0]] and live_ref.scores(Q, D).dtype == np.float64
    assert live_ref.pack([1, 0, 0, 1]).tolist() == [9] and live_ref.pack([0] * 31 + [1, 1]).tolist() == [-2 ** 31, 1]
