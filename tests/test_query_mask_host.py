"""Corpus search with a row filter per query, host side: the workspace sizing and the pre-launch errors of
gdr_sim_topk's GDR_SIM_QUERY_MASK mode, the pinned ABI and ops.QueryRows on the CPU.  Needs no GPU."""
import ctypes as C
import hashlib

import numpy as np
import pytest
import torch

import live_ref
from gdr_amd import _ffi, ops

# (B, N, k) -> gdr_sim_topk_workspace_bytes(B, N, d, k, flags) for flags 0 and GDR_SIM_EXHAUSTIVE, as tests/test_live_search_host.py
# records them from before either mask mode existed
PLAIN = {
    (8, 70_001, 10): (640_256, 4_613_376),
    (512, 320_000, 100): (130_615_296, 1_310_787_584),
    (4, 1000, 10): (99_072, 99_072),
    (40, 2_800_003, 8192): (239_785_216, 896_046_336),
}
QM = 8


def test_flag_value_and_pinned_abi():
    assert _ffi.SIM_QUERY_MASK == QM
    assert _ffi.SIM_QUERY_MASK & (_ffi.SIM_EXHAUSTIVE | _ffi.SIM_NO_STREAM | _ffi.SIM_LIVE_MASK) == 0
    assert _ffi.lib().gdr_abi_version() == 9 == _ffi.ABI_VERSION
    name = lambda t: getattr(t, "__name__", str(t))   # noqa: E731
    text = ";".join(f"{k}:{name(r)}({','.join(name(a) for a in args)})" for k, (r, args) in sorted(_ffi.SIGNATURES.items()))
    assert len(_ffi.SIGNATURES) == 75
    assert hashlib.sha256(text.encode()).hexdigest() == "290bf61378c8afa411523c3af82231a508b23b22da2603b6645954cc9845c9c2"


@pytest.mark.parametrize("B,N,k", list(PLAIN))
def test_workspace_is_the_size_for_the_other_flags_plus_one_bitmap_per_query(B, N, k):
    """Fails without the feature: bit 8 of flags was ignored, so the flagged size was the plain one."""
    l = _ffi.lib()
    for d in (64, 768):
        for f in (0, _ffi.SIM_EXHAUSTIVE, _ffi.SIM_NO_STREAM):
            plain = l.gdr_sim_topk_workspace_bytes(B, N, d, k, f)
            assert plain == PLAIN[(B, N, k)][1 if f == _ffi.SIM_EXHAUSTIVE else 0], "the unflagged size moved"
            assert l.gdr_sim_topk_workspace_bytes(B, N, d, k, f | QM) - plain == B * live_ref.mask_bytes(N)
        # the live mask's own size is what it was
        assert l.gdr_sim_topk_workspace_bytes(B, N, d, k, _ffi.SIM_LIVE_MASK) - PLAIN[(B, N, k)][0] == live_ref.mask_bytes(N)
    assert l.gdr_sim_topk_workspace_bytes(0, N, 64, k, QM) == 0


def test_flagged_call_refuses_a_short_workspace_before_any_launch():
    """The pointers are never dereferenced.  A buffer of the unflagged size and one a byte short are GDR_ENOSPC at every shape."""
    l = _ffi.lib()
    p, ws = C.c_void_p(256), C.c_void_p(4096)
    for (B, N, k) in PLAIN:
        for fn in (l.gdr_sim_topk, l.gdr_sim_topk_bf16):
            for more in (0, _ffi.SIM_EXHAUSTIVE, _ffi.SIM_NO_STREAM):
                flags = QM | more
                plain = l.gdr_sim_topk_workspace_bytes(B, N, 64, k, more)
                need = l.gdr_sim_topk_workspace_bytes(B, N, 64, k, flags)
                assert need == plain + B * live_ref.mask_bytes(N)
                for nbytes in (plain, need - 1):
                    assert fn(p, B, p, N, 64, k, 0, p, p, None, flags, ws, nbytes, None) == _ffi.GDR_ENOSPC, (B, N, k, flags, nbytes)
                    msg = l.gdr_last_error()
                    assert str(need).encode() in msg and str(nbytes).encode() in msg, msg


def test_both_masks_in_one_call_and_a_misaligned_workspace_are_refused():
    l = _ffi.lib()
    p, ws = C.c_void_p(256), C.c_void_p(4096)
    for fn in (l.gdr_sim_topk, l.gdr_sim_topk_bf16):
        for more in (0, _ffi.SIM_EXHAUSTIVE):
            assert fn(p, 8, p, 70_001, 64, 10, 0, p, p, None, _ffi.SIM_LIVE_MASK | QM | more, ws, 1 << 40, None) == _ffi.GDR_EINVAL
            msg = l.gdr_last_error()
            assert b"GDR_SIM_LIVE_MASK" in msg and b"GDR_SIM_QUERY_MASK" in msg and b"AND" in msg, msg
    assert l.gdr_sim_topk(p, 8, p, 70_001, 64, 10, 0, p, p, None, QM, C.c_void_p(4096 + 128), 1 << 30, None) == _ffi.GDR_EINVAL
    assert b"256-byte aligned" in l.gdr_last_error()


def test_header_documents_the_flag_and_the_unmasked_prefilter():
    import os
    from conftest import REPO
    text = open(os.path.join(REPO, "include", "gdr_hip.h")).read()
    assert "#define GDR_SIM_QUERY_MASK 8" in text
    assert "#define GDR_SIM_LIVE_MASK 4" in text
    assert "stays UNMASKED" in text


# ---------------------------------------------------------------------------------------------- ops.QueryRows (CPU device)
def _packed(x):
    return np.stack([live_ref.pack(r) for r in x])


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 1000, 4097])
def test_query_rows_against_bool_arrays(B, n):
    rng = np.random.default_rng(100 * B + n)
    x = rng.random((B, n)) < 0.5
    x[:, -1] = True                                                       # the last row: bit (n - 1) % 32, bit 31 at n = 32
    if n > 31:
        x[0, 31] = True                                                   # bit 31 of word 0: the sign bit of the int32
        x[-1, :31] = False
    R = ops.QueryRows.from_bool(torch.from_numpy(x))
    assert (R.B, R.n) == (B, n) and R.words.dtype == torch.int32 and tuple(R.words.shape) == (B, -(-n // 32))
    assert np.array_equal(R.words.numpy(), _packed(x))
    assert np.array_equal(R.to_bool().numpy(), x)
    assert R.counts().dtype == torch.int64 and R.counts().tolist() == x.sum(1).tolist()
    if n > 31:
        assert int(R.words[0, 0]) < 0 and int(R.words[-1, 0]) == (-2 ** 31 if x[-1, 31] else 0)
    # from_allowed / from_denied give the same bitmaps from id lists (repeats allowed), on host tensors, lists and arrays
    ids = [np.nonzero(r)[0] for r in x]
    A = ops.QueryRows.from_allowed([torch.from_numpy(np.concatenate([i, i[:1]])) for i in ids], n)
    assert np.array_equal(A.words.numpy(), _packed(x))
    Dn = ops.QueryRows.from_denied([np.nonzero(~r)[0].tolist() for r in x], n)
    assert np.array_equal(Dn.words.numpy(), _packed(x)) and Dn.counts().tolist() == x.sum(1).tolist()
    # garbage past n in the last word is ignored by the readers
    if n % 32:
        R._words[:, -1] |= torch.tensor(np.int32(-1) << np.int32(n % 32))
        assert R.counts().tolist() == x.sum(1).tolist() and np.array_equal(R.to_bool().numpy(), x)
    # and_ with the live rows, in place; rows() copies a sub-batch
    live = rng.random(n) < 0.7
    L = ops.LiveRows.from_bool(torch.from_numpy(live))
    assert A.and_(L) is A
    assert np.array_equal(A.to_bool().numpy(), x & live) and A.counts().tolist() == (x & live).sum(1).tolist()
    pick = [B - 1, 0, B - 1]
    S = Dn.rows(pick)
    assert (S.B, S.n) == (3, n) and np.array_equal(S.to_bool().numpy(), x[pick])
    S.and_(L)
    assert np.array_equal(Dn.to_bool().numpy(), x), "rows() must copy"


def test_query_rows_empty_and_errors():
    e = ops.QueryRows(3, 70, "cpu")
    assert tuple(e.words.shape) == (3, 3) and not e.to_bool().any() and e.counts().tolist() == [0, 0, 0]
    assert ops.QueryRows.from_allowed([[], [5], []], 70).counts().tolist() == [0, 1, 0]
    assert ops.QueryRows.from_denied([[], [5, 5], [0, 69]], 70).counts().tolist() == [70, 69, 68]
    for make in (ops.QueryRows.from_allowed, ops.QueryRows.from_denied):
        for bad in ([-1], [70], torch.tensor([3, 70])):
            with pytest.raises(_ffi.GdrError, match=r"\[0, 70\)"):
                make([[1], bad], 70)
    with pytest.raises(_ffi.GdrError, match="LiveRows over the same 70 rows"):
        e.and_(ops.LiveRows(71, "cpu"))
    with pytest.raises(_ffi.GdrError, match=r"bool \[B, n\]"):
        ops.QueryRows.from_bool(torch.zeros(5, dtype=torch.bool))


def test_sim_topk_validates_allowed_before_anything_runs():
    Q, D = torch.zeros(2, 8), torch.zeros(40, 8)
    with pytest.raises(_ffi.GdrError, match="CUDA"):
        ops.sim_topk(Q, D, 3, allowed=ops.QueryRows(2, 40, "cpu"))
