"""CPU checks of document removal / update: the restatement (tests/lifecycle_ref.py) against hand-written cases,
the argument validation of gdr_cluster_insert's removal mode (new_target == NULL) before any launch, and the host-side refusals
of ops.cluster_remove.  No call below reaches a launch: each one ends in validation or at the workspace-size check that
follows it."""
import ctypes as C

import numpy as np
import pytest
import torch

import lifecycle_ref


def test_restatement_on_hand_written_cases():
    offs = np.array([0, 3, 3, 7, 8], np.int32)                 # clusters {5, 2, 9}, {}, {1, 8, 0, 4}, {7}
    mem = np.array([5, 2, 9, 1, 8, 0, 4, 7], np.int32)
    o, m, n = lifecycle_ref.remove(offs, mem, [2])
    assert o.tolist() == [0, 2, 2, 6, 7] and m.tolist() == [5, 9, 1, 8, 0, 4, 7] and n == 1
    o, m, n = lifecycle_ref.remove(offs, mem, [0, 1, 3, 6, 9])  # 3 and 6 are in no cluster: ignored; order kept
    assert o.tolist() == [0, 2, 2, 4, 5] and m.tolist() == [5, 2, 8, 4, 7] and n == 3
    o, m, n = lifecycle_ref.remove(offs, mem, [7])              # a cluster that loses every member stays, empty
    assert o.tolist() == [0, 3, 3, 7, 7] and m.tolist() == [5, 2, 9, 1, 8, 0, 4] and n == 1
    o, m, n = lifecycle_ref.remove(offs, mem, np.arange(10))
    assert o.tolist() == [0, 0, 0, 0, 0] and m.size == 0 and n == 8 and o.dtype == np.int32 and m.dtype == np.int32
    o, m, n = lifecycle_ref.remove(offs, mem, [])
    assert np.array_equal(o, offs) and np.array_equal(m, mem) and n == 0
    # update: 9 moves to the empty cluster, 0 stays where it is (now behind the others), 6 (in no cluster) joins cluster 0
    o, m = lifecycle_ref.update(offs, mem, [0, 6, 9], [2, 0, 1])
    assert o.tolist() == [0, 3, 4, 8, 9] and m.tolist() == [5, 2, 6, 9, 1, 8, 4, 0, 7]


def test_removal_mode_passes_argument_validation_without_gpu():
    """Fails on the parent commit, which answers GDR_EINVAL ("null new_ids / new_target") to new_target == NULL."""
    from gdr_amd import _ffi
    l = _ffi.lib()
    p = C.c_void_p(16)                   # never dereferenced: every call ends before a launch
    err = lambda: l.gdr_last_error()     # noqa: E731
    ws = l.gdr_cluster_insert_workspace_bytes(100)
    # the workspace-size check follows every argument check: a call that answers GDR_ENOSPC has passed them all
    ok = lambda **kw: dict(dict(off=p, mem=p, C=100, n_old=50, ids=p, tgt=None, n=5, map=None, n_map=0, oo=p, om=p, mx=p,   # noqa: E731
                                ws=p, wsb=ws - 1), **kw)

    def ins(a):
        return l.gdr_cluster_insert(a["off"], a["mem"], a["C"], a["n_old"], a["ids"], a["tgt"], a["n"], a["map"], a["n_map"],
                                    a["oo"], a["om"], a["mx"], a["ws"], a["wsb"], None)
    assert ins(ok()) == _ffi.GDR_ENOSPC and b"workspace" in err()
    assert ins(ok(wsb=0)) == _ffi.GDR_ENOSPC
    assert ins(ok(n_old=(1 << 31) - 3)) == _ffi.GDR_ENOSPC          # nothing is added: n_new does not count against 2^31
    # the mode takes no target_map
    assert ins(ok(map=p, n_map=4)) == _ffi.GDR_EINVAL and b"target_map" in err()
    assert ins(ok(map=p, n_map=0)) == _ffi.GDR_EINVAL and b"target_map" in err()
    assert ins(ok(map=None, n_map=4)) == _ffi.GDR_EINVAL and b"target_map" in err()
    # n = 0 is what it is today with or without new_target: nothing to insert, nothing to remove, arguments accepted
    assert ins(ok(n=0)) == _ffi.GDR_ENOSPC and ins(ok(n=0, tgt=p)) == _ffi.GDR_ENOSPC
    assert ins(ok(n=0, ids=None)) == _ffi.GDR_ENOSPC
    assert ins(ok(n=0, map=p, n_map=0)) == _ffi.GDR_EINVAL and b"target_map" in err()
    # what failed before still fails
    assert ins(ok(ids=None)) == _ffi.GDR_EINVAL and b"null new_ids" in err()
    assert ins(ok(ids=None, tgt=p)) == _ffi.GDR_EINVAL
    assert ins(ok(n=-1)) == _ffi.GDR_EINVAL
    assert ins(ok(off=None)) == _ffi.GDR_EINVAL and b"null" in err()
    assert ins(ok(mem=None)) == _ffi.GDR_EINVAL
    assert ins(ok(om=None)) == _ffi.GDR_EINVAL and ins(ok(mx=None)) == _ffi.GDR_EINVAL
    assert ins(ok(C=0)) == _ffi.GDR_EINVAL and b"bad size" in err()
    assert ins(ok(n_old=-1)) == _ffi.GDR_EINVAL
    assert ins(ok(ws=None)) == _ffi.GDR_EINVAL
    # the ABI did not move
    assert l.gdr_cluster_insert_workspace_bytes(100) == ws and l.gdr_abi_version() == 9


def test_cluster_remove_refuses_bad_lists_without_gpu():
    from gdr_amd import _ffi, ops
    i32 = lambda *a: torch.tensor(a, dtype=torch.int32)   # noqa: E731   CPU tensors: a call that got past the checks would raise "need CUDA"
    offs, mem = i32(0, 2, 4), i32(3, 1, 0, 2)
    for bad in (i32(2, 1), i32(1, 1), i32(0, 3, 3)):
        with pytest.raises(_ffi.GdrError, match="strictly ascending"):
            ops.cluster_remove(offs, mem, bad)
    with pytest.raises(_ffi.GdrError, match="int32"):
        ops.cluster_remove(offs, mem, torch.tensor([1, 2]))
    with pytest.raises(_ffi.GdrError, match="int32"):
        ops.cluster_remove(offs.long(), mem, i32(1))
    with pytest.raises(_ffi.GdrError, match="int32"):
        ops.cluster_remove(offs, mem.to(torch.int16), i32(1))
    with pytest.raises(_ffi.GdrError, match="CUDA"):      # a well-formed call gets as far as the device check
        ops.cluster_remove(offs, mem, i32(1, 2))
