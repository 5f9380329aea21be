"""Hierarchical k-means docids, host side: the numpy restatement tests/kmeans_ref.py against the reference's golden
(g15: the reference's kmeans.py run on a fixture with every fit_predict recorded, and sklearn's Lloyd from a fixed C0), the integer
hash shared by the restatement and the device module, and the argument checks of the C ABI that need no GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import kmeans_ref as kr
from conftest import golden


@pytest.fixture(scope="module")
def g15():
    return golden("g15_kmeans")


def test_id_rules_reproduce_the_reference_mapping(g15):
    """(a) fed the reference's recorded labels node by node, the restated id assembly gives the reference's id mapping: class
    digits, the rank digit of a 2..c leaf, no rank digit for a leaf of one doc."""
    g = g15
    N, k, c = g["X"].shape[0], int(g["k"]), int(g["c"])
    off = g["call_offsets"]
    by_rows = {}
    for i in range(len(off) - 1):
        r, lab = g["call_rows"][off[i]:off[i + 1]].astype(np.int64), g["call_labels"][off[i]:off[i + 1]]
        by_rows[np.sort(r).tobytes()] = (r, lab)
    used = []

    def recorded(ids, level, path):
        r, lab = by_rows[np.asarray(ids, np.int64).tobytes()]
        used.append(len(ids))
        out = np.empty(len(ids), np.int64)
        out[np.searchsorted(ids, r)] = lab
        return out

    digits, leaves = kr.assemble_ids(N, k, c, recorded)
    got, lens = kr.pad_digits(digits)
    assert len(used) == len(off) - 1, "not every recorded split was visited"
    assert np.array_equal(lens, g["ref_lengths"]) and np.array_equal(got, g["ref_digits"])
    sizes = np.array([len(m) for _p, m in leaves])
    assert (sizes == 1).any() and (sizes <= c).all(), "the fixture is meant to hold a singleton leaf"
    for path, mem in leaves:                       # the singleton rule: a leaf of one doc has no rank digit
        assert all(len(digits[m]) == len(path) + (len(mem) > 1) for m in mem)


def test_restated_lloyd_equals_sklearn(g15):
    """(b) from the same C0 the float64 restatement gives sklearn's labels exactly and its centres and inertia."""
    g = g15
    X = g["X"].astype(np.float64)
    assert float(g["lloyd_min_gap"]) >= float(g["gap_bound"])
    for T in g["T_list"]:
        lab, cen, inertia, _rounds = kr.lloyd(X, g["C0"], int(T))
        assert np.array_equal(lab, g[f"sk_labels_T{T}"]), f"labels differ from sklearn at T={T}"
        assert np.abs(cen - g[f"sk_centers_T{T}"]).max() < 1e-12
        assert abs(inertia - float(g[f"sk_inertia_T{T}"])) <= 1e-9 * inertia


def test_default_n_init_is_what_the_quality_table_says(g15):
    from gdr_amd import kmeans
    g = g15
    ok = [int(n) for n, r in zip(g["n_inits"], g["pooled_inertia_ratio"]) if r <= 1.05]
    assert ok and kmeans.DEFAULT_N_INIT == ok[0] == int(g["default_n_init"])
    assert float(g["build_min_gap_n1"]) >= float(g["gap_bound"]) and float(g["build_min_gap_default"]) >= float(g["gap_bound"])
    assert float(g["restart_lead_default"]) >= 1e-4


def test_mix_agrees_between_numpy_and_torch():
    from gdr_amd import kmeans
    ids = np.concatenate([np.arange(4096), [2 ** 31 - 1, 123456789, 2 ** 31 - 2]]).astype(np.int64)
    for seed, r, lvl in [(7, 0, 0), (7, 3, 2), (2 ** 40 + 5, 15, 7), (0, 0, 0), (2 ** 63 + 11, 1, 1)]:
        a = kr.mix(seed, r, lvl, ids)
        b = kmeans.mix_keys(seed, r, lvl, torch.from_numpy(ids)).numpy()
        assert np.array_equal(a, b) and (a >= 0).all()
    assert kr.splitmix64(0) == 0xE220A8397B1DCDAF          # the published first output of splitmix64 seeded with 0


def test_restatement_rules_on_small_cases():
    rng = np.random.default_rng(0)
    # rule 6: identical rows terminate; 100 docs, k = 4, c = 6 -> 25 -> 7/6/6/6 -> 2/2/2/1
    X = np.tile(rng.standard_normal(8).astype(np.float32), (100, 1))
    digits, leaves = kr.build(X, 4, 6, n_init=2)
    assert len({tuple(x) for x in digits}) == 100 and max(len(m) for _p, m in leaves) <= 6
    assert sorted(np.concatenate([m for _p, m in leaves]).tolist()) == list(range(100))
    # the root is split even when it has <= c docs; a node with fewer docs than k leaves the other children absent
    X = rng.standard_normal((5, 8)).astype(np.float32)
    digits, leaves = kr.build(X, 8, 30)
    assert all(len(x) >= 1 for x in digits) and len(leaves) <= 5
    # ids longer than max_depth are refused
    X = rng.standard_normal((300, 8)).astype(np.float32)
    with pytest.raises(ValueError, match="max_depth"):
        kr.build(X, 2, 2, max_depth=3)
    # an emptied child keeps its centroid and does not exist in the tree
    X = rng.standard_normal((60, 8)).astype(np.float32)
    C0 = np.concatenate([X[:3].astype(np.float64), 100.0 * np.ones((1, 8))])
    lab, cen, _i, _r = kr.lloyd(X, C0, 20)
    assert (lab != 3).all() and np.array_equal(cen[3], C0[3])
    digits, _leaves = kr.build(X, 4, 30, init_centroids=C0)
    assert all(x[0] != 3 for x in digits)


def test_c_abi_refuses_bad_arguments_without_a_gpu():
    """N >= 2^31, d and k outside the supported range and a short workspace are refused before anything is launched."""
    from gdr_amd import _ffi
    lib = _ffi.lib()
    buf = (C.c_char * 4096)()
    p = C.cast(buf, C.c_void_p)

    def assign(N=1000, d=32, n_rows=10, k=8, ws=4096):
        return lib.gdr_kmeans_assign(p, N, d, p, n_rows, p, 1, p, k, p, 1, None, p, p, p, p, p, ws, None)

    def err():
        return lib.gdr_last_error().decode()

    assert assign(N=1 << 31) == _ffi.GDR_EINVAL and "int32 doc ids" in err()
    assert assign(d=30) == _ffi.GDR_EINVAL and "d=30" in err()
    assert assign(d=4100) == _ffi.GDR_EINVAL and "d=4100" in err()
    assert assign(k=1) == _ffi.GDR_EINVAL and "k=1" in err()
    assert assign(k=65) == _ffi.GDR_EINVAL and "k=65" in err()
    assert assign(ws=0) == _ffi.GDR_ENOSPC and "workspace" in err()
    assert lib.gdr_kmeans_partition(p, p, 1 << 31, p, 1, 8, p, 1, p, p, p, p, 4096, None) == _ffi.GDR_EINVAL
    assert lib.gdr_kmeans_partition(p, p, 10, p, 1, 65, p, 1, p, p, p, p, 4096, None) == _ffi.GDR_EINVAL and "k=65" in err()
    assert lib.gdr_kmeans_assign_tile() == 128 and lib.gdr_kmeans_partition_tile() == 256
    assert lib.gdr_kmeans_assign_workspace_bytes(3, 30) >= 3 * 30 * 4
    assert lib.gdr_kmeans_centroids(p, 1000, 30, p, p, 10, 2, p, p, p, 1 << 20, None) == _ffi.GDR_EINVAL and "d=30" in err()
    assert lib.gdr_kmeans_centroids(p, 1000, 32, p, p, 1000, 2, p, p, p, 16, None) == _ffi.GDR_ENOSPC
    assert lib.gdr_kmeans_centroids_workspace_bytes(1000, 32) >= 2 * 4 * 32 * 4
