"""CPU checks of corpus expansion: the host restatement against the reference's golden (g14), argument
validation of gdr_cluster_centroids / gdr_cluster_insert before any launch, the CLI flags and the clusters.npz round trip."""
import numpy as np
import pytest

import expand_ref
from conftest import golden


def test_restatement_equals_reference_golden():
    g = golden("g14_expand")
    D, docnum = g["D"], int(g["docnum"])
    cent, counts = expand_ref.centroids(D, g["offsets"], g["members"])
    assert np.array_equal(cent.view(np.uint32), g["ref_centroids"].view(np.uint32)), "centroids not bit-identical"
    assert (counts == 0).sum() == 2 and (cent[counts == 0] == 0).all()
    tgt, gap, band = expand_ref.assign(D[docnum:], cent, counts)
    assert (gap > band).all() and np.allclose(gap, g["gap"])
    assert (counts[tgt] > 0).all()
    offs, mem = expand_ref.merge(g["offsets"], g["members"], np.arange(docnum, D.shape[0]), tgt)
    assert expand_ref.as_sets(offs, mem) == expand_ref.as_sets(g["exp_offsets"], g["exp_members"])
    # member order: existing members first (as given), then the inserted ones ascending
    for c in range(len(offs) - 1):
        old = g["members"][g["offsets"][c]:g["offsets"][c + 1]]
        seg = mem[offs[c]:offs[c + 1]]
        assert np.array_equal(seg[:old.size], old) and np.all(np.diff(seg[old.size:]) > 0)


def test_sorted_members_is_the_tree_order():
    from gdr_amd import codec
    g = golden("g14_expand")
    idx = codec.ClusterIndex([str(x) for x in g["names"]], g["offsets"], g["members"])
    s = idx.sorted_members()
    for c in range(len(idx.names)):
        lo, hi = idx.offsets[c], idx.offsets[c + 1]
        assert np.array_equal(s[lo:hi], np.sort(idx.members[lo:hi]))
    assert np.array_equal(idx.unassigned(0, g["D"].shape[0]), np.arange(int(g["docnum"]), g["D"].shape[0]))


def test_entry_points_reject_bad_arguments_without_gpu():
    import ctypes as C
    from gdr_amd import _ffi
    l = _ffi.lib()
    p = C.c_void_p(16)                   # never dereferenced: every call below must fail validation before a launch
    err = lambda: l.gdr_last_error()     # noqa: E731
    assert l.gdr_cluster_centroids(None, 10, 64, p, p, 10, 3, p, p, None) == _ffi.GDR_EINVAL and b"null" in err()
    assert l.gdr_cluster_centroids(p, 10, 64, p, None, 10, 3, p, p, None) == _ffi.GDR_EINVAL
    assert l.gdr_cluster_centroids(p, -1, 64, p, p, 10, 3, p, p, None) == _ffi.GDR_EINVAL and b"bad size" in err()
    assert l.gdr_cluster_centroids(p, 10, 64, p, p, -1, 3, p, p, None) == _ffi.GDR_EINVAL
    assert l.gdr_cluster_centroids(p, 10, 64, p, p, 10, 0, p, p, None) == _ffi.GDR_EINVAL
    assert l.gdr_cluster_centroids(p, 1 << 31, 64, p, p, 10, 3, p, p, None) == _ffi.GDR_EINVAL and b"int32" in err()
    for d in (0, 6, 4100, -4):
        assert l.gdr_cluster_centroids(p, 10, d, p, p, 10, 3, p, p, None) == _ffi.GDR_EINVAL and b"d=" in err()
    q = C.c_void_p(20)                   # 4-byte but not 16-byte aligned: the kernel reads D / writes centroids as float4
    assert l.gdr_cluster_centroids(q, 10, 64, p, p, 10, 3, p, p, None) == _ffi.GDR_EINVAL and b"aligned" in err()
    assert l.gdr_cluster_centroids(p, 10, 64, p, p, 10, 3, q, p, None) == _ffi.GDR_EINVAL and b"aligned" in err()
    ws = l.gdr_cluster_insert_workspace_bytes(100)
    assert ws >= 800 and l.gdr_cluster_insert_workspace_bytes(0) == 0
    ok = lambda **kw: dict(dict(off=p, mem=p, C=100, n_old=50, ids=p, tgt=p, n=5, map=None, n_map=0, oo=p, om=p, mx=p,   # noqa: E731
                                ws=p, wsb=ws), **kw)

    def ins(a):
        return l.gdr_cluster_insert(a["off"], a["mem"], a["C"], a["n_old"], a["ids"], a["tgt"], a["n"], a["map"], a["n_map"],
                                    a["oo"], a["om"], a["mx"], a["ws"], a["wsb"], None)
    assert ins(ok(off=None)) == _ffi.GDR_EINVAL and b"null" in err()
    assert ins(ok(mem=None)) == _ffi.GDR_EINVAL
    assert ins(ok(ids=None)) == _ffi.GDR_EINVAL
    assert ins(ok(mx=None)) == _ffi.GDR_EINVAL
    assert ins(ok(C=0)) == _ffi.GDR_EINVAL and b"bad size" in err()
    assert ins(ok(n_old=-1)) == _ffi.GDR_EINVAL
    assert ins(ok(n=-1)) == _ffi.GDR_EINVAL
    assert ins(ok(n_old=(1 << 31) - 3, n=5)) == _ffi.GDR_EINVAL and b"int32" in err()
    assert ins(ok(map=p, n_map=0)) == _ffi.GDR_EINVAL and b"target_map" in err()
    assert ins(ok(map=None, n_map=4)) == _ffi.GDR_EINVAL
    assert ins(ok(ws=None)) == _ffi.GDR_EINVAL
    assert ins(ok(wsb=ws - 1)) == _ffi.GDR_ENOSPC and b"workspace" in err()


def test_cli_flags_parse():
    from gdr_amd import main as gmain
    a = gmain.parsers_parser([])
    assert a.expand_index == 0 and a.save_index == ""
    a = gmain.parsers_parser(["--expand_index", "1", "--save_index", "/tmp/x/clusters.npz", "--docnum", "300"])
    assert a.expand_index == 1 and a.save_index == "/tmp/x/clusters.npz" and a.docnum == 300


def test_cli_refuses_expand_with_several_gpus():
    from gdr_amd import main as gmain
    with pytest.raises(SystemExit, match="expand_index"):
        gmain.main(["--mode", "eval", "--expand_index", "1", "--n_gpu", "2"])


def test_save_npz_round_trip(tmp_path):
    from gdr_amd import codec
    g = golden("g14_expand")
    idx = codec.ClusterIndex([str(x) for x in g["names"]], g["exp_offsets"], g["exp_members"])
    path = tmp_path / "clusters_expanded"                # no .npz suffix: written to exactly this path
    idx.save_npz(str(path))
    z = np.load(str(path), allow_pickle=False)
    assert sorted(z.files) == ["cluster_members", "cluster_names", "cluster_offsets"]
    back = codec.ClusterIndex([str(x) for x in z["cluster_names"]], z["cluster_offsets"], z["cluster_members"])
    assert back.names == idx.names and np.array_equal(back.offsets, idx.offsets) and np.array_equal(back.members, idx.members)
    merged = idx.with_csr(g["offsets"], g["members"])
    assert merged.names == idx.names and merged[idx.names[0]] == g["members"][:g["offsets"][1]].tolist()
    with pytest.raises(ValueError):
        idx.with_csr(g["offsets"][:-1], g["members"])
